// The host half of ance_pack_tokens_by_id -- argument checks, parameter fill, refusals before any launch -- as a stand-alone program
// for a host sanitizer (make -C ance_amd/csrc host-sanitize).  Refusal paths only: no call here reaches a launch, no device is
// needed, and the device pointers are fake and never dereferenced.  Every message is compared whole.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>

#include "../../../include/ance_amd.h"

static int failures = 0;

static void expect(int rc, const char *why) {
    const std::string want = std::string("ance_pack_tokens_by_id: invalid argument (") + why + ")";
    const char *msg = ance_last_error();
    if (rc != ANCE_E_INVALID || want != msg) {
        printf("FAIL: wanted '%s', got %d '%s'\n", want.c_str(), rc, msg);
        ++failures;
    }
}

static AncePackByIdArgs good() {
    int32_t *fake = (int32_t *)(uintptr_t)0x10000;
    AncePackByIdArgs a = {};
    a.ids = fake; a.d_seq_len = fake; a.d_seq_off = fake; a.d_seq_kept = fake; a.d_dropped = (int64_t *)fake;
    a.packed_ids = fake; a.packed_positions = fake;
    a.n_seq = 3; a.L = 40; a.rows = 90; a.padding_idx = 1; a.vocab = 32769; a.max_pos = 514;
    return a;
}

int main() {
    int32_t *odd2 = (int32_t *)(uintptr_t)0x10002;
    expect(ance_pack_tokens_by_id(nullptr, nullptr), "null pointer");
#define REFUSED(why, edit)                                 \
    do {                                                   \
        AncePackByIdArgs a = good();                       \
        edit;                                              \
        expect(ance_pack_tokens_by_id(&a, nullptr), why);  \
    } while (0)
    REFUSED("null pointer", a.ids = nullptr);
    REFUSED("null pointer", a.d_seq_len = nullptr);
    REFUSED("null pointer", a.d_seq_off = nullptr);
    REFUSED("null pointer", a.d_seq_kept = nullptr);
    REFUSED("null pointer", a.d_dropped = nullptr);
    REFUSED("null pointer", a.packed_ids = nullptr);
    REFUSED("null pointer", a.packed_positions = nullptr);
    REFUSED("alignment: an integer array is not 4-byte aligned", a.ids = odd2);
    REFUSED("alignment: an integer array is not 4-byte aligned", a.d_seq_len = odd2);
    REFUSED("alignment: an integer array is not 4-byte aligned", a.d_seq_off = odd2);
    REFUSED("alignment: an integer array is not 4-byte aligned", a.d_seq_kept = odd2);
    REFUSED("alignment: an integer array is not 4-byte aligned", a.packed_ids = odd2);
    REFUSED("alignment: an integer array is not 4-byte aligned", a.packed_positions = odd2);
    REFUSED("alignment: d_dropped is not 8-byte aligned", a.d_dropped = (int64_t *)(uintptr_t)0x10004);
    REFUSED("n_seq outside 1 .. 65535", a.n_seq = 0);
    REFUSED("n_seq outside 1 .. 65535", a.n_seq = 65536);
    REFUSED("L outside 1 .. 512", a.L = 0);
    REFUSED("L outside 1 .. 512", a.L = 513);
    REFUSED("rows < 1", a.rows = 0);
    REFUSED("rows < 1", a.rows = -7);
    REFUSED("an empty table", a.vocab = 0);
    REFUSED("an empty table", a.max_pos = 0);
    REFUSED("padding_idx outside 0 .. vocab - 1", a.padding_idx = -1);
    REFUSED("padding_idx outside 0 .. vocab - 1", a.padding_idx = 32769);
#undef REFUSED
    printf(failures ? "%d refusal(s) missing\n" : "every refusal made on the host (%d missing)\n", failures);
    return failures ? 1 : 0;
}
