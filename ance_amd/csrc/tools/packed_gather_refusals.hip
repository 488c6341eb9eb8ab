// The host halves of ance_record_lengths and ance_gather_batch_packed -- argument checks, parameter fill, refusals before any launch --
// as a stand-alone program for a host sanitizer (make -C ance_amd/csrc host-sanitize).  Refusal paths only: no call here reaches a
// launch, no device is needed, and the device pointers are fake and never dereferenced.
#include <cstdint>
#include <cstdio>
#include <cstring>

#include "../../../include/ance_amd.h"

static int failures = 0;

static void expect(int rc, const char *fn, const char *why) {
    const char *msg = ance_last_error();
    if (rc != ANCE_E_INVALID || !strstr(msg, fn) || !strstr(msg, why)) {
        printf("FAIL: wanted a refusal of %s with '%s', got %d '%s'\n", fn, why, rc, msg);
        ++failures;
    }
}

static AncePackedGatherSegment good() {
    void *fake = (void *)(uintptr_t)0x10000;
    AncePackedGatherSegment s = {};
    s.d_records = fake; s.n_records = 9;
    s.d_index = (const int64_t *)fake; s.n_index = 20;
    s.d_cum = (const int64_t *)fake;
    s.packed_ids = (int32_t *)fake; s.packed_positions = (int32_t *)fake;
    s.d_seq_off = (int32_t *)fake; s.d_seq_kept = (int32_t *)fake; s.d_dropped = (int64_t *)fake;
    s.L = 2048; s.chunk_len = 512; s.rows = 90;
    s.position_mode = ANCE_EMBED_POSITION_ROBERTA; s.padding_idx = 1; s.vocab = 1000; s.max_pos = 514;
    return s;
}

int main() {
    const char *g = "ance_gather_batch_packed", *r = "ance_record_lengths";
    void *fake = (void *)(uintptr_t)0x10000, *odd2 = (void *)(uintptr_t)0x10002, *odd4 = (void *)(uintptr_t)0x10004;
    AncePackedGatherSegment segs[3];

    expect(ance_gather_batch_packed(nullptr, 1, 0, 4, nullptr, nullptr), g, "null segment table");
    for (int n : {0, -1, 4}) {
        segs[0] = good();
        expect(ance_gather_batch_packed(segs, n, 0, 4, nullptr, nullptr), g, "n_segs");
    }
    segs[0] = segs[1] = segs[2] = good();
    expect(ance_gather_batch_packed(segs, 3, 0, 0, nullptr, nullptr), g, "B < 1");
    expect(ance_gather_batch_packed(segs, 3, -1, 4, nullptr, nullptr), g, "first < 0");
    expect(ance_gather_batch_packed(segs, 3, 17, 4, nullptr, nullptr), g, "past the item index");
    expect(ance_gather_batch_packed(segs, 3, 0, 4, (const int64_t *)odd4, nullptr), g, "d_first");
    expect(ance_gather_batch_packed(segs, 3, 0, 16384, (const int64_t *)fake, nullptr), g, "65535");  // four chunks each

#define REFUSED(why, edit)                                                             \
    do {                                                                               \
        for (int which = 0; which < 3; ++which) {                                      \
            segs[0] = segs[1] = segs[2] = good();                                      \
            AncePackedGatherSegment &s = segs[which];                                  \
            edit;                                                                      \
            expect(ance_gather_batch_packed(segs, 3, 0, 4, nullptr, nullptr), g, why); \
        }                                                                              \
    } while (0)
    REFUSED("null pointer", s.d_records = nullptr);
    REFUSED("null pointer", s.d_index = nullptr);
    REFUSED("null pointer", s.d_cum = nullptr);
    REFUSED("null pointer", s.packed_ids = nullptr);
    REFUSED("null pointer", s.packed_positions = nullptr);
    REFUSED("null pointer", s.d_seq_off = nullptr);
    REFUSED("null pointer", s.d_seq_kept = nullptr);
    REFUSED("null pointer", s.d_dropped = nullptr);
    REFUSED("4-byte aligned", s.d_records = odd2);
    REFUSED("4-byte aligned", s.packed_ids = (int32_t *)odd2);
    REFUSED("4-byte aligned", s.d_seq_kept = (int32_t *)odd2);
    REFUSED("8-byte aligned", s.d_index = (const int64_t *)odd4);
    REFUSED("8-byte aligned", s.d_cum = (const int64_t *)odd4);
    REFUSED("8-byte aligned", s.d_dropped = (int64_t *)odd4);
    REFUSED("n_records", s.n_records = 0);
    REFUSED("n_index", s.n_index = -1);
    REFUSED("past the item index", s.n_index = 3);
    REFUSED("L < 1", s.L = 0);
    REFUSED("chunk_len", s.chunk_len = 0);
    REFUSED("chunk_len", s.chunk_len = 1024);
    REFUSED("does not divide", s.chunk_len = 500);
    REFUSED("too large", s.n_index = INT64_MAX / 8);
    REFUSED("rows", s.rows = 0);
    REFUSED("rows", s.rows = -7);
    REFUSED("empty table", s.vocab = 0);
    REFUSED("empty table", s.max_pos = 0);
    REFUSED("position_mode", s.position_mode = 2);
    REFUSED("padding_idx", s.padding_idx = -1);
    REFUSED("padding_idx", s.padding_idx = 1000);
    REFUSED("padding_idx", (s.position_mode = ANCE_EMBED_POSITION_ABSOLUTE, s.padding_idx = -2));
#undef REFUSED

    expect(ance_record_lengths(nullptr, 9, 2048, 512, 0, (int32_t *)fake, nullptr), r, "null pointer");
    expect(ance_record_lengths(fake, 9, 2048, 512, 0, nullptr, nullptr), r, "null pointer");
    expect(ance_record_lengths(odd2, 9, 2048, 512, 0, (int32_t *)fake, nullptr), r, "aligned");
    expect(ance_record_lengths(fake, 9, 2048, 512, 0, (int32_t *)odd2, nullptr), r, "aligned");
    expect(ance_record_lengths(fake, 0, 2048, 512, 0, (int32_t *)fake, nullptr), r, "n_records");
    expect(ance_record_lengths(fake, 9, 0, 512, 0, (int32_t *)fake, nullptr), r, "L < 1");
    expect(ance_record_lengths(fake, 9, 2048, 0, 0, (int32_t *)fake, nullptr), r, "chunk_len");
    expect(ance_record_lengths(fake, 9, 2048, 2048, 0, (int32_t *)fake, nullptr), r, "chunk_len");
    expect(ance_record_lengths(fake, 9, 2048, 500, 0, (int32_t *)fake, nullptr), r, "does not divide");
    expect(ance_record_lengths(fake, 9, 2048, 512, 2, (int32_t *)fake, nullptr), r, "rule");
    expect(ance_record_lengths(fake, INT64_MAX / 2, 2048, 512, 0, (int32_t *)fake, nullptr), r, "too large");

    printf(failures ? "%d refusal(s) missing\n" : "every refusal made on the host (%d missing)\n", failures);
    return failures ? 1 : 0;
}
