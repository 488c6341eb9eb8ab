// The host halves of ance_lamb_step_scaled, ance_adamw_step_scaled and ance_loss_scale_update -- argument checks and refusals before
// any launch -- as a stand-alone program for a host sanitizer (make -C ance_amd/csrc host-sanitize).  Refusal paths only: no call
// here reaches a launch, no device is needed, and the device pointers are fake and never dereferenced.  Every message is compared
// whole.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <string>

#include "../../../include/ance_amd.h"

static int failures = 0;

static void expect(const char *fn, int rc, const char *why) {
    const std::string want = std::string(fn) + ": invalid argument (" + why + ")";
    const char *msg = ance_last_error();
    if (rc != ANCE_E_INVALID || want != msg) {
        printf("FAIL: wanted '%s', got %d '%s'\n", want.c_str(), rc, msg);
        ++failures;
    }
}

// the arguments of a step that would launch; the tests below spoil one at a time
struct Step {
    int n_tensors = 7, n_groups = 2, adam = 0;  // adam: correct_bias for AdamW
    int64_t n_chunks = 9;
    double max_grad_norm = 1.0;
    float *scale = (float *)(uintptr_t)0x10000, *flag = (float *)(uintptr_t)0x10010, *prev = nullptr;
    float *norm = (float *)(uintptr_t)0x10020, *out = (float *)(uintptr_t)0x10100;
    int64_t *skipped = (int64_t *)(uintptr_t)0x10030;
    void *ws = (void *)(uintptr_t)0x20000;
    size_t ws_bytes = (size_t)1 << 30;
};

static int lamb(const Step &a) {
    return ance_lamb_step_scaled(a.n_tensors, a.n_groups, a.n_chunks, a.adam, a.max_grad_norm, a.scale, a.flag, a.prev, a.norm, a.skipped,
                                 a.out, a.ws, a.ws_bytes, nullptr);
}
static int adamw(const Step &a) {
    return ance_adamw_step_scaled(a.n_tensors, a.n_groups, a.n_chunks, a.adam, a.max_grad_norm, a.scale, a.flag, a.norm, a.skipped, a.ws,
                                  a.ws_bytes, nullptr);
}

int main() {
    const char *LAMB = "ance_lamb_step_scaled", *ADAMW = "ance_adamw_step_scaled", *UPDATE = "ance_loss_scale_update";
#define REFUSED(why, edit)               \
    do {                                 \
        Step a;                          \
        edit;                            \
        expect(LAMB, lamb(a), why);      \
        expect(ADAMW, adamw(a), why);    \
    } while (0)
    // what the planned forms refuse
    REFUSED("table sizes out of range", a.n_tensors = 0);
    REFUSED("table sizes out of range", a.n_tensors = -3);
    REFUSED("table sizes out of range", a.n_groups = 0);
    REFUSED("table sizes out of range", a.n_chunks = -1);
    REFUSED("table sizes out of range", a.n_chunks = (int64_t)INT32_MAX + 1);
    REFUSED("max_grad_norm not 0 or a positive finite number", a.max_grad_norm = -1.0);
    REFUSED("max_grad_norm not 0 or a positive finite number", a.max_grad_norm = (double)INFINITY);
    REFUSED("max_grad_norm not 0 or a positive finite number", a.max_grad_norm = (double)NAN);
    REFUSED("null d_grad_norm", a.norm = nullptr);
    REFUSED("null or unaligned workspace", a.ws = nullptr);
    REFUSED("null or unaligned workspace", a.ws = (void *)(uintptr_t)0x20008);
    REFUSED("workspace too small", a.ws_bytes = 0);
    REFUSED("workspace too small", a.ws_bytes = 64);
    // what the scaled forms add, with and without the clip (d_grad_norm may then be null: it is not the reason)
    REFUSED("null d_grad_scale", a.scale = nullptr);
    REFUSED("null d_found_inf", a.flag = nullptr);
    REFUSED("null d_grad_scale", a.max_grad_norm = 0.0; a.norm = nullptr; a.scale = nullptr);
    REFUSED("null d_found_inf", a.max_grad_norm = 0.0; a.norm = nullptr; a.flag = nullptr);
#undef REFUSED
    {
        // without the clip the workspace is still the clipped one: the size the unclipped planned step accepts is refused
        Step a;
        a.max_grad_norm = 0.0;
        a.norm = nullptr;
        a.ws_bytes = ance_lamb_workspace_bytes(a.n_tensors, a.n_groups, 2 * 16384);  // 9 chunks
        expect(LAMB, lamb(a), "workspace too small");
        a.ws_bytes = ance_adamw_workspace_bytes(a.n_tensors, a.n_groups, 2 * 16384, 0);
        expect(ADAMW, adamw(a), "workspace too small");
        a.out = nullptr;
        a.ws_bytes = (size_t)1 << 30;
        expect(LAMB, lamb(a), "null d_out");
    }

    float *scale = (float *)(uintptr_t)0x10000, *flag = (float *)(uintptr_t)0x10010;
    int32_t *tracker = (int32_t *)(uintptr_t)0x10020;
    expect(UPDATE, ance_loss_scale_update(nullptr, tracker, flag, 2.0, 0.5, 2000, nullptr), "null pointer");
    expect(UPDATE, ance_loss_scale_update(scale, nullptr, flag, 2.0, 0.5, 2000, nullptr), "null pointer");
    expect(UPDATE, ance_loss_scale_update(scale, tracker, nullptr, 2.0, 0.5, 2000, nullptr), "null pointer");
    expect(UPDATE, ance_loss_scale_update((float *)(uintptr_t)0x10002, tracker, flag, 2.0, 0.5, 2000, nullptr), "unaligned pointer");
    expect(UPDATE, ance_loss_scale_update(scale, (int32_t *)(uintptr_t)0x10021, flag, 2.0, 0.5, 2000, nullptr), "unaligned pointer");
    expect(UPDATE, ance_loss_scale_update(scale, tracker, (float *)(uintptr_t)0x10013, 2.0, 0.5, 2000, nullptr), "unaligned pointer");
    const double bad[] = {0.0, -2.0, (double)INFINITY, (double)NAN};
    for (double f : bad) {
        expect(UPDATE, ance_loss_scale_update(scale, tracker, flag, f, 0.5, 2000, nullptr), "growth_factor not a positive finite number");
        expect(UPDATE, ance_loss_scale_update(scale, tracker, flag, 2.0, f, 2000, nullptr), "backoff_factor not a positive finite number");
    }
    expect(UPDATE, ance_loss_scale_update(scale, tracker, flag, 2.0, 0.5, 0, nullptr), "growth_interval < 1");
    expect(UPDATE, ance_loss_scale_update(scale, tracker, flag, 2.0, 0.5, -5, nullptr), "growth_interval < 1");

    printf(failures ? "%d refusal(s) missing\n" : "every refusal made on the host (%d missing)\n", failures);
    return failures ? 1 : 0;
}
