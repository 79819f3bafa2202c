// Host build of audio-codec_amd/csrc/body_index.h: the three phases of pacx_index_body with loops in
// place of lanes (the segment maps' pointer jumping included, double-buffered as in k_index.hip),
// driven through ctypes by tests/test_index_model.py.
#include <stdint.h>
#include <string.h>

#include <vector>

#include "body_index.h"

extern "C" int ixc_segment_bytes(void) { return PACX_IX_SEG; }
extern "C" int ixc_max_record(void) { return PACX_IX_MAX_RECORD; }

// offsets / n_bytes: max_records entries; result: 3 words.  Returns the number of segments.
extern "C" long long ixc_index_body(const uint8_t *body, long long n_body, int n_channels, int final, long long max_records,
                                    long long *offsets, int32_t *n_bytes, long long *result)
{
    const long long n_seg = pacx_ix_segments(n_body), n_groups = pacx_ix_groups(n_seg);
    std::vector<uint32_t> tab((size_t)n_seg * PACX_IX_ENTRIES);
    std::vector<uint8_t> by(PACX_IX_SEG + 4);
    std::vector<uint32_t> nd[2] = {std::vector<uint32_t>(PACX_IX_SEG), std::vector<uint32_t>(PACX_IX_SEG)};
    for (long long s = 0; s < n_seg; ++s) {                                  // phase 1: k_index_segments
        const long long seg0 = s * PACX_IX_SEG;
        for (int i = 0; i < PACX_IX_SEG + 4; ++i)
            by[i] = seg0 + i < n_body ? body[seg0 + i] : (uint8_t)0;
        for (int p = 0; p < PACX_IX_SEG; ++p)
            nd[0][p] = pacx_ix_node(p, seg0 + p, n_body, pacx_ix_le32(by.data() + p));
        int cur = 0;
        for (int r = 0; r < PACX_IX_ROUNDS; ++r) {
            for (int p = 0; p < PACX_IX_SEG; ++p) {
                uint32_t a = nd[cur][p];
                if (pacx_ix_kind(a) == PACX_IX_JUMP)
                    a = pacx_ix_jump(a, nd[cur][pacx_ix_pos(a)]);
                nd[cur ^ 1][p] = a;
            }
            cur ^= 1;
        }
        for (int e = 0; e < PACX_IX_ENTRIES; ++e)
            tab[(size_t)s * PACX_IX_ENTRIES + e] = nd[cur][e];
    }
    std::vector<uint64_t> gtab((size_t)n_groups * PACX_IX_ENTRIES);           // phase 2a: k_index_compose
    for (long long g = 0; g < n_groups; ++g)
        for (int e = 0; e < PACX_IX_ENTRIES; ++e)
            gtab[(size_t)g * PACX_IX_ENTRIES + e] = pacx_ix_compose_lane(tab.data(), n_seg, g, e);
    std::vector<int32_t> gentry(n_groups), entry(n_seg);
    std::vector<long long> gbase(n_groups), base(n_seg);
    long long fin[3];
    pacx_ix_stitch(gtab.data(), n_groups, n_channels, final, max_records, gentry.data(), gbase.data(), fin);   // 2b
    result[0] = fin[0];
    if (fin[1] >= 0)
        result[1] = fin[1];
    result[2] = fin[2];
    for (long long g = 0; g < n_groups; ++g)                                  // phase 2c: k_index_fill
        pacx_ix_fill_group(tab.data(), n_seg, g, gentry[g], gbase[g], entry.data(), base.data());
    for (long long s = 0; s < n_seg; ++s)                                     // phase 3: k_index_emit
        pacx_ix_emit_segment(body, n_body, s, entry[s], base[s], fin[0], fin[1] < 0, offsets, n_bytes, result + 1);
    return n_seg;
}
