// The host front end of the BertLayer seams (layer_tail_common.h behind layer_tail.hip and layer_tail_half.hip) -- the conversion of
// the fp32 structs, the argument checks, refusals before any launch -- as a stand-alone program for a host sanitizer
// (make -C ance_amd/csrc host-sanitize).  Both entry families through the public entry points, refusal paths only: no call here reaches a launch, no device is needed, and the device pointers
// are fake and never dereferenced.
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../../../include/ance_amd.h"

static int failures = 0;
static void *const fake = (void *)(uintptr_t)0x10000, *const odd = (void *)(uintptr_t)0x10004;

// the whole reason, between the parentheses of "fn: invalid argument (why)"
static void expect(int rc, const char *fn, const char *why) {
    const char *msg = ance_last_error();
    char want[160];
    snprintf(want, sizeof(want), "(%s)", why);
    if (rc != ANCE_E_INVALID || strstr(msg, fn) != msg || !strstr(msg, want)) {
        printf("FAIL: wanted a refusal of %s with '%s', got %d '%s'\n", fn, why, rc, msg);
        ++failures;
    }
}

static const char *STRIDE32 = "stride: not a multiple of 4 or below the width";
static const char *STRIDE16 = "stride: a 16-bit row stride is not a multiple of 8 or below the width";
static const char *DTYPE = "dtype neither ANCE_DTYPE_F16 nor ANCE_DTYPE_BF16";

// 17 rows: one workgroup and one row, stats 512 bytes, one tail partial row 3 * 768 * 4 bytes
static AnceLayerTailArgs tail32() {
    AnceLayerTailArgs a = {};
    a.x = a.res = a.bias = a.gamma = a.beta = (const float *)fake;
    a.y = (float *)fake;
    a.ld_x = a.ld_res = a.ld_y = a.H = 768;
    a.n_rows = 17;
    a.eps = 1e-5f; a.dropout_p = 0.1f; a.training = 1;
    a.d_workspace = fake; a.workspace_bytes = 512 + 2 * 3 * 768 * 4;
    return a;
}
static AnceLayerTailGradArgs tail32_grads() {
    AnceLayerTailGradArgs g = {};
    g.dy = (const float *)fake;
    g.dx = g.dres = g.dgamma = g.dbeta = g.dbias = (float *)fake;
    g.ld_dy = g.ld_dx = g.ld_dres = 768;
    return g;
}
static AnceLayerTail16Args tail16() {
    AnceLayerTail16Args a = {};
    a.x = fake; a.y16 = fake;
    a.res = a.bias = a.gamma = a.beta = (const float *)fake;
    a.y = (float *)fake;
    a.ld_x = a.ld_res = a.ld_y = a.ld_y16 = a.H = 768;
    a.n_rows = 17;
    a.dtype = ANCE_DTYPE_F16;
    a.eps = 1e-5f; a.dropout_p = 0.1f; a.training = 1;
    a.d_workspace = fake; a.workspace_bytes = 512 + 2 * 3 * 768 * 4;
    return a;
}
static AnceLayerTail16GradArgs tail16_grads() {
    AnceLayerTail16GradArgs g = {};
    g.dy = (const float *)fake; g.dy16 = fake; g.dx = fake;
    g.dres = g.dgamma = g.dbeta = g.dbias = (float *)fake;
    g.ld_dy = g.ld_dy16 = g.ld_dx = g.ld_dres = 768;
    return g;
}
static AnceBiasGeluArgs gelu32() {
    AnceBiasGeluArgs a = {};
    a.x = a.bias = (const float *)fake;
    a.y = (float *)fake;
    a.ld_x = a.ld_y = a.N = 3072;
    a.n_rows = 17;
    a.d_workspace = fake; a.workspace_bytes = 2 * 3072 * 4;
    return a;
}
static AnceBiasGeluGradArgs gelu32_grads() {
    AnceBiasGeluGradArgs g = {};
    g.dy = (const float *)fake;
    g.dx = g.dbias = (float *)fake;
    g.ld_dy = g.ld_dx = 3072;
    return g;
}
static AnceBiasGelu16Args gelu16() {
    AnceBiasGelu16Args a = {};
    a.x = fake; a.y = fake;
    a.bias = (const float *)fake;
    a.ld_x = a.ld_y = a.N = 3072;
    a.n_rows = 17;
    a.dtype = ANCE_DTYPE_BF16;
    a.d_workspace = fake; a.workspace_bytes = 2 * 3072 * 4;
    return a;
}
static AnceBiasGelu16GradArgs gelu16_grads() {
    AnceBiasGelu16GradArgs g = {};
    g.dy = fake; g.dx = fake;
    g.dbias = (float *)fake;
    g.ld_dy = g.ld_dx = 3072;
    return g;
}

int main() {
    const uint64_t *odd_stream = (const uint64_t *)(uintptr_t)0x10008;

    // the fp32 tail: forward and backward share the argument edits; G edits the gradients
#define T32(why, edit)                                                                                                      \
    do {                                                                                                                    \
        AnceLayerTailArgs a = tail32();                                                                                     \
        AnceLayerTailGradArgs g = tail32_grads();                                                                           \
        (void)g;                                                                                                            \
        edit;                                                                                                               \
        expect(ance_layer_tail_forward(&a, nullptr), "ance_layer_tail_forward:", why);                                \
        expect(ance_layer_tail_forward_dstream(&a, nullptr, nullptr), "ance_layer_tail_forward_dstream:", why);       \
        expect(ance_layer_tail_backward(&a, &g, nullptr), "ance_layer_tail_backward:", why);                          \
        expect(ance_layer_tail_backward_dstream(&a, &g, nullptr, nullptr), "ance_layer_tail_backward_dstream:", why); \
    } while (0)
#define T32_BWD(why, edit)                                                                         \
    do {                                                                                           \
        AnceLayerTailArgs a = tail32();                                                            \
        AnceLayerTailGradArgs g = tail32_grads();                                                  \
        edit;                                                                                      \
        expect(ance_layer_tail_backward(&a, &g, nullptr), "ance_layer_tail_backward:", why); \
    } while (0)
    T32("width H not 768 or 1024", a.H = 512);
    T32("n_rows < 1", a.n_rows = 0);
    T32("null pointer", a.x = nullptr);
    T32("alignment: a base is not 16-byte aligned", a.x = (const float *)odd);
    T32(STRIDE32, a.ld_x = 770);
    T32(STRIDE32, a.ld_x = 764);
    T32("null pointer", a.res = nullptr);
    T32(STRIDE32, a.ld_res = 774);
    T32("alignment: a base is not 16-byte aligned", a.bias = (const float *)odd);
    T32("null pointer", a.gamma = nullptr);
    T32("dropout_p outside [0, 1)", a.dropout_p = 1.0f);
    T32("eps <= 0", a.eps = 0.0f);
    T32("null or unaligned workspace", a.d_workspace = nullptr);
    T32("workspace too small", a.workspace_bytes = 511);
    T32("n_rows < 1", (a.n_rows = 0, a.x = nullptr));  // precedence: the shape before the pointers
    T32_BWD("workspace too small", a.workspace_bytes = 512);  // the forward's share alone
    T32_BWD("null pointer", g.dy = nullptr);                  // the fp32 family's text, not the 16-bit family's
    T32_BWD(STRIDE32, g.ld_dy = 770);
    T32_BWD(STRIDE32, g.ld_dx = 2);
    T32_BWD(STRIDE32, g.ld_dres = 770);
    T32_BWD("alignment: a base is not 16-byte aligned", g.dgamma = (float *)odd);
    T32_BWD("alignment: a base is not 16-byte aligned", g.dbias = (float *)odd);
    T32_BWD("eps <= 0", (a.eps = -1.0f, g.dy = nullptr));     // the arguments before the gradients
    {
        AnceLayerTailArgs a = tail32();
        AnceLayerTailGradArgs g = tail32_grads();
        expect(ance_layer_tail_forward(nullptr, nullptr), "ance_layer_tail_forward:", "null pointer");
        expect(ance_layer_tail_backward(nullptr, &g, nullptr), "ance_layer_tail_backward:", "null pointer");
        expect(ance_layer_tail_backward(&a, nullptr, nullptr), "ance_layer_tail_backward:", "null pointer");
        expect(ance_layer_tail_forward_dstream(nullptr, odd_stream, nullptr), "ance_layer_tail_forward_dstream:", "alignment: d_stream is not 16-byte aligned");
        expect(ance_layer_tail_backward_dstream(&a, &g, odd_stream, nullptr), "ance_layer_tail_backward_dstream:", "alignment: d_stream is not 16-byte aligned");
        a.y = nullptr; a.beta = nullptr;  // not the backward's: it goes on to the gradients
        g.dy = (const float *)odd;
        expect(ance_layer_tail_backward(&a, &g, nullptr), "ance_layer_tail_backward:", "alignment: a base is not 16-byte aligned");
        expect(ance_layer_tail_forward(&a, nullptr), "ance_layer_tail_forward:", "null pointer");
    }
#undef T32
#undef T32_BWD

    // the 16-bit tail
#define T16(why, edit)                                                                                                          \
    do {                                                                                                                        \
        AnceLayerTail16Args a = tail16();                                                                                       \
        AnceLayerTail16GradArgs g = tail16_grads();                                                                             \
        (void)g;                                                                                                                \
        edit;                                                                                                                   \
        expect(ance_layer_tail16_forward(&a, nullptr), "ance_layer_tail16_forward:", why);                                \
        expect(ance_layer_tail16_forward_dstream(&a, nullptr, nullptr), "ance_layer_tail16_forward_dstream:", why);       \
        expect(ance_layer_tail16_backward(&a, &g, nullptr), "ance_layer_tail16_backward:", why);                          \
        expect(ance_layer_tail16_backward_dstream(&a, &g, nullptr, nullptr), "ance_layer_tail16_backward_dstream:", why); \
    } while (0)
#define T16_BWD(why, edit)                                                                             \
    do {                                                                                               \
        AnceLayerTail16Args a = tail16();                                                              \
        AnceLayerTail16GradArgs g = tail16_grads();                                                    \
        edit;                                                                                          \
        expect(ance_layer_tail16_backward(&a, &g, nullptr), "ance_layer_tail16_backward:", why); \
    } while (0)
    T16("width H not 768 or 1024", a.H = 3072);
    T16("n_rows < 1", a.n_rows = -3);
    T16(DTYPE, a.dtype = ANCE_DTYPE_F32);
    T16(DTYPE, a.dtype = 3);
    T16(DTYPE, a.dtype = -1);
    T16(DTYPE, a.dtype = 32);
    T16(DTYPE, a.dtype = 1 << 30);
    T16("n_rows < 1", (a.n_rows = 0, a.dtype = ANCE_DTYPE_F32));  // after n_rows ...
    T16(DTYPE, (a.dtype = ANCE_DTYPE_F32, a.x = nullptr));        // ... and before x
    T16("null pointer", a.x = nullptr);
    T16(STRIDE16, a.ld_x = 772);   // a multiple of 4 will not do for 16-bit rows
    T16(STRIDE16, a.ld_x = 760);
    T16(STRIDE32, a.ld_res = 770);
    T16("null pointer", a.gamma = nullptr);
    T16("dropout_p outside [0, 1)", a.dropout_p = -0.5f);
    T16("workspace too small", a.workspace_bytes = 8);
    {
        AnceLayerTail16Args a = tail16();
        a.ld_y = 770;
        expect(ance_layer_tail16_forward(&a, nullptr), "ance_layer_tail16_forward:", STRIDE32);   // y is an fp32 matrix
        a = tail16(); a.ld_y16 = 772;
        expect(ance_layer_tail16_forward(&a, nullptr), "ance_layer_tail16_forward:", STRIDE16);
        a = tail16(); a.y16 = nullptr; a.ld_y16 = 0; a.beta = nullptr;   // y16 is optional; beta is not
        expect(ance_layer_tail16_forward(&a, nullptr), "ance_layer_tail16_forward:", "null pointer");
        expect(ance_layer_tail16_forward(nullptr, nullptr), "ance_layer_tail16_forward:", "null pointer");
        expect(ance_layer_tail16_backward(&a, nullptr, nullptr), "ance_layer_tail16_backward:", "null pointer");
        expect(ance_layer_tail16_forward_dstream(&a, odd_stream, nullptr), "ance_layer_tail16_forward_dstream:", "alignment: d_stream is not 16-byte aligned");
    }
    T16_BWD("null pointer: neither dy nor dy16", (g.dy = nullptr, g.dy16 = nullptr));
    T16_BWD(STRIDE32, (g.ld_dy = 772 + 2, g.dy16 = nullptr));
    T16_BWD(STRIDE16, (g.ld_dy16 = 772, g.dy = nullptr));
    T16_BWD(STRIDE16, g.ld_dx = 772);
    T16_BWD(STRIDE32, g.ld_dres = 2);
    T16_BWD("alignment: a base is not 16-byte aligned", g.dbeta = (float *)odd);
#undef T16
#undef T16_BWD

    // bias + GELU, both families
#define G32(why, edit)                                                                            \
    do {                                                                                          \
        AnceBiasGeluArgs a = gelu32();                                                            \
        AnceBiasGeluGradArgs g = gelu32_grads();                                                  \
        (void)g;                                                                                  \
        edit;                                                                                     \
        expect(ance_bias_gelu_forward(&a, nullptr), "ance_bias_gelu_forward:", why);        \
        expect(ance_bias_gelu_backward(&a, &g, nullptr), "ance_bias_gelu_backward:", why);  \
    } while (0)
#define G32_BWD(why, edit)                                                                        \
    do {                                                                                          \
        AnceBiasGeluArgs a = gelu32();                                                            \
        AnceBiasGeluGradArgs g = gelu32_grads();                                                  \
        edit;                                                                                     \
        expect(ance_bias_gelu_backward(&a, &g, nullptr), "ance_bias_gelu_backward:", why);  \
    } while (0)
    G32("width N not 3072 or 4096", a.N = 768);
    G32("n_rows < 1", a.n_rows = 0);
    G32("null pointer", a.x = nullptr);
    G32(STRIDE32, a.ld_x = 3074);
    G32("null pointer", a.bias = nullptr);
    G32_BWD("null or unaligned workspace", a.d_workspace = nullptr);
    G32_BWD("workspace too small", a.workspace_bytes = 3072 * 4);
    G32_BWD("workspace too small", (a.workspace_bytes = 0, g.dy = nullptr));   // the workspace before the gradients ...
    G32_BWD("null pointer", (a.bias = nullptr, a.workspace_bytes = 0));       // ... and after the arguments
    G32_BWD("null pointer", g.dy = nullptr);
    G32_BWD(STRIDE32, g.ld_dy = 3070);
    G32_BWD(STRIDE32, g.ld_dx = 3074);
    G32_BWD("alignment: a base is not 16-byte aligned", g.dbias = (float *)odd);
    {
        AnceBiasGeluArgs a = gelu32();
        a.ld_y = 3074;
        expect(ance_bias_gelu_forward(&a, nullptr), "ance_bias_gelu_forward:", STRIDE32);
        expect(ance_bias_gelu_forward(nullptr, nullptr), "ance_bias_gelu_forward:", "null pointer");
        expect(ance_bias_gelu_backward(&a, nullptr, nullptr), "ance_bias_gelu_backward:", "null pointer");
    }
#undef G32
#undef G32_BWD
#define G16(why, edit)                                                                                \
    do {                                                                                              \
        AnceBiasGelu16Args a = gelu16();                                                              \
        AnceBiasGelu16GradArgs g = gelu16_grads();                                                    \
        (void)g;                                                                                      \
        edit;                                                                                         \
        expect(ance_bias_gelu16_forward(&a, nullptr), "ance_bias_gelu16_forward:", why);        \
        expect(ance_bias_gelu16_backward(&a, &g, nullptr), "ance_bias_gelu16_backward:", why);  \
    } while (0)
#define G16_BWD(why, edit)                                                                            \
    do {                                                                                              \
        AnceBiasGelu16Args a = gelu16();                                                              \
        AnceBiasGelu16GradArgs g = gelu16_grads();                                                    \
        edit;                                                                                         \
        expect(ance_bias_gelu16_backward(&a, &g, nullptr), "ance_bias_gelu16_backward:", why);  \
    } while (0)
    G16("width N not 3072 or 4096", a.N = 1024);
    G16(DTYPE, a.dtype = ANCE_DTYPE_F32);
    G16(DTYPE, a.dtype = 7);
    G16("n_rows < 1", (a.n_rows = 0, a.dtype = ANCE_DTYPE_F32));
    G16(DTYPE, (a.dtype = ANCE_DTYPE_F32, a.x = nullptr));
    G16(STRIDE16, a.ld_x = 3076);
    G16("null pointer", a.bias = nullptr);
    G16_BWD("workspace too small", a.workspace_bytes = 100);
    G16_BWD("null pointer", g.dy = nullptr);
    G16_BWD(STRIDE16, g.ld_dy = 3076);
    G16_BWD(STRIDE16, g.ld_dx = 3076);
    {
        AnceBiasGelu16Args a = gelu16();
        a.ld_y = 3076;
        expect(ance_bias_gelu16_forward(&a, nullptr), "ance_bias_gelu16_forward:", STRIDE16);
        expect(ance_bias_gelu16_forward(nullptr, nullptr), "ance_bias_gelu16_forward:", "null pointer");
        expect(ance_bias_gelu16_backward(&a, nullptr, nullptr), "ance_bias_gelu16_backward:", "null pointer");
    }
#undef G16
#undef G16_BWD

    // the queries answer 0 for what is not supported, the same in both families
    if (ance_layer_tail_workspace_bytes(17, 768) != 512 + 2 * 3 * 768 * 4 || ance_layer_tail16_workspace_bytes(17, 768) != 512 + 2 * 3 * 768 * 4 ||
        ance_bias_gelu_workspace_bytes(17, 3072) != 2 * 3072 * 4 || ance_bias_gelu16_workspace_bytes(17, 3072) != 2 * 3072 * 4 ||
        ance_layer_tail_workspace_bytes(0, 768) || ance_layer_tail16_workspace_bytes(17, 512) || ance_bias_gelu_workspace_bytes(17, 768) ||
        ance_bias_gelu16_workspace_bytes((int64_t)1 << 31, 3072) || ance_layer_tail_rows_per_workgroup() != ANCE_LAYER_TAIL_ROWS_PER_WORKGROUP) {
        printf("FAIL: a workspace query\n");
        ++failures;
    }

    printf(failures ? "%d refusal(s) missing\n" : "every refusal made on the host (%d missing)\n", failures);
    return failures ? 1 : 0;
}
