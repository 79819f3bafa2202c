/*
 * body_index.h -- the record index of a .pac body ('<L nBytes' + payload, back to back), written
 * once for device (hipcc, k_index.hip) and host (g++, tests/hostcheck/index_check.cpp) builds.
 *
 * The chain of length prefixes is serial by definition.  It is indexed in three phases whose every
 * loop has a trip count fixed by the constants below or by the number of segments:
 *
 *   1. segment maps   one workgroup per segment of PACX_IX_SEG bytes: for every byte position p the
 *                     node "where does a walk that starts at p leave this segment, and after how many
 *                     records" (pointer jumping in LDS, PACX_IX_ROUNDS rounds); kept for the
 *                     PACX_IX_ENTRIES offsets at which a record of the previous segment can end;
 *   2. stitch         groups of PACX_IX_GROUP segments are composed for every entry offset
 *                     (pacx_ix_compose_lane), the groups are walked by one lane (pacx_ix_stitch) and
 *                     filled in in parallel (pacx_ix_fill_group): entry offset and first record
 *                     number of every segment, one dependent load per GROUP on the serial part;
 *   3. emit           one lane per segment walks its own records from its entry offset and writes
 *                     offsets / sizes at its first record number (pacx_ix_emit_segment).
 *
 * The input is untrusted bytes: every prefix is classified by pacx_ix_node alone, every index is
 * checked against its array, and nothing at or past body + n_body is read.
 */
#ifndef PACX_BODY_INDEX_H
#define PACX_BODY_INDEX_H

#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define PACX_IX_HD __host__ __device__ __forceinline__
#else
#define PACX_IX_HD static inline
#endif

#define PACX_IX_SEG 8192                            /* bytes of a segment: a power of two >= 4096 */
#define PACX_IX_MAX_RECORD 2192                     /* = PACX_PAYLOAD_STRIDE (k_index.hip asserts it): longest payload */
#define PACX_IX_ENTRIES (PACX_IX_MAX_RECORD + 4)    /* offsets at which a segment can be entered   */
#define PACX_IX_MAX_CHAIN (PACX_IX_SEG / 5 + 1)     /* records that start in one segment, at most  */
#define PACX_IX_ROUNDS 12                           /* 2^(ROUNDS-1) >= MAX_CHAIN + 1               */
#define PACX_IX_GROUP 64                            /* segments composed into one group            */

/* a node: low 16 bits = kind << 13 | position, high 16 bits = records passed on the way there */
#define PACX_IX_JUMP 0u         /* position = next prefix inside the segment                        */
#define PACX_IX_EXIT 1u         /* position = offset of the next prefix in the NEXT segment         */
#define PACX_IX_BAD 2u          /* position = a prefix whose length is outside 1..MAX_RECORD        */
#define PACX_IX_INCOMPLETE 3u   /* position = a prefix (or its record) that runs past n_body        */
#define PACX_IX_END 4u          /* position = n_body                                                */

PACX_IX_HD uint32_t pacx_ix_kind(uint32_t node) { return (node >> 13) & 7u; }
PACX_IX_HD uint32_t pacx_ix_pos(uint32_t node) { return node & 8191u; }
PACX_IX_HD uint32_t pacx_ix_count(uint32_t node) { return node >> 16; }
PACX_IX_HD uint32_t pacx_ix_make(uint32_t kind, uint32_t pos, uint32_t count)
{
    return (count << 16) | (kind << 13) | (pos & 8191u);
}

/* the rule for ONE prefix: position p of its segment, g = its position in the body, len = the four
   bytes at g as '<L' (only looked at when they lie inside the body) */
PACX_IX_HD uint32_t pacx_ix_node(int p, long long g, long long n_body, uint32_t len)
{
    if (g == n_body)
        return pacx_ix_make(PACX_IX_END, (uint32_t)p, 0);
    if (g > n_body)
        return pacx_ix_make(PACX_IX_BAD, (uint32_t)p, 0);             /* never on a chain */
    if (g + 4 > n_body)
        return pacx_ix_make(PACX_IX_INCOMPLETE, (uint32_t)p, 0);
    if (len < 1u || len > (uint32_t)PACX_IX_MAX_RECORD)
        return pacx_ix_make(PACX_IX_BAD, (uint32_t)p, 0);
    if (g + 4 + (long long)len > n_body)
        return pacx_ix_make(PACX_IX_INCOMPLETE, (uint32_t)p, 0);
    const int q = p + 4 + (int)len;
    if (q < PACX_IX_SEG)
        return pacx_ix_make(PACX_IX_JUMP, (uint32_t)q, 1);
    return pacx_ix_make(PACX_IX_EXIT, (uint32_t)(q - PACX_IX_SEG), 1);
}

/* one round of pointer jumping: node a followed by the node at a's target */
PACX_IX_HD uint32_t pacx_ix_jump(uint32_t a, uint32_t at_target)
{
    return ((pacx_ix_count(a) + pacx_ix_count(at_target)) << 16) | (at_target & 0xFFFFu);
}

PACX_IX_HD uint32_t pacx_ix_le32(const uint8_t *b)
{
    return (uint32_t)b[0] | ((uint32_t)b[1] << 8) | ((uint32_t)b[2] << 16) | ((uint32_t)b[3] << 24);
}

PACX_IX_HD long long pacx_ix_segments(long long n_body) { return n_body / PACX_IX_SEG + 1; }   /* n_body itself has a node */
PACX_IX_HD long long pacx_ix_groups(long long n_seg) { return (n_seg + PACX_IX_GROUP - 1) / PACX_IX_GROUP; }

/* a group node: bits 0-15 the node's kind and position, bits 16-31 the segment (of the group) that
   position belongs to (EXIT: the group's last), bits 32-63 the records passed */
PACX_IX_HD uint64_t pacx_ix_gmake(uint32_t node16, uint32_t seg_in_group, uint64_t count)
{
    return (count << 32) | ((uint64_t)(seg_in_group & 0xFFFFu) << 16) | (node16 & 0xFFFFu);
}

/* phase 2a, lane (group, entry): walk the group's segment tables from entry offset e */
PACX_IX_HD uint64_t pacx_ix_compose_lane(const uint32_t *tab, long long n_seg, long long group, int e)
{
    uint64_t count = 0;
    uint32_t node = pacx_ix_make(PACX_IX_EXIT, (uint32_t)e, 0), seg = 0;
    for (int k = 0; k < PACX_IX_GROUP; ++k) {
        const long long s = group * PACX_IX_GROUP + k;
        if (s >= n_seg || pacx_ix_kind(node) != PACX_IX_EXIT)
            continue;
        uint32_t at = pacx_ix_pos(node);
        if (at >= (uint32_t)PACX_IX_ENTRIES)              /* cannot happen: a record is at most MAX_RECORD long */
            at = PACX_IX_ENTRIES - 1;
        node = tab[s * PACX_IX_ENTRIES + at];
        count += pacx_ix_count(node);
        seg = (uint32_t)k;
    }
    return pacx_ix_gmake(node, seg, count);
}

/* what a call returns, from the whole chain's length, its terminal and the caller's limits */
struct PacxIxResult {
    long long n_records;      /* returned: a multiple of n_channels                               */
    long long consumed;       /* position of the first prefix not returned, or -1 when a lane of
                                 phase 3 has to supply it (n_records < chain)                     */
    long long error_at;       /* position of the prefix at which the chain broke, or -1           */
};

PACX_IX_HD PacxIxResult pacx_ix_finish(long long chain, uint32_t kind, long long terminal_at, int n_channels, int final,
                                       long long max_records)
{
    PacxIxResult r;
    long long n = chain;
    r.error_at = -1;
    if (chain >= max_records)
        n = max_records;                                  /* the walk stops here, before whatever follows */
    else if (kind == PACX_IX_BAD || kind == PACX_IX_EXIT || (kind == PACX_IX_INCOMPLETE && final))
        r.error_at = terminal_at;                         /* EXIT: a walk cannot leave the last segment */
    r.n_records = n - n % n_channels;
    r.consumed = r.n_records == chain ? terminal_at : -1;
    return r;
}

/* phase 2b, one lane: the groups in order.  gentry[g] / gbase[g]: entry offset and first record number
   of group g.  fin[0..2]: records returned, consumed (or -1), error position. */
PACX_IX_HD void pacx_ix_stitch(const uint64_t *gtab, long long n_groups, int n_channels, int final, long long max_records,
                               int32_t *gentry, long long *gbase, long long *fin)
{
    uint32_t e = 0, kind = PACX_IX_EXIT;
    long long base = 0, at = 0;
    for (long long g = 0; g < n_groups; ++g) {
        gentry[g] = kind == PACX_IX_EXIT ? (int32_t)e : -1;          /* -1: the chain ended before this group */
        gbase[g] = base;
        if (kind != PACX_IX_EXIT)
            continue;
        const uint64_t t = gtab[g * PACX_IX_ENTRIES + (e < (uint32_t)PACX_IX_ENTRIES ? e : PACX_IX_ENTRIES - 1)];
        base += (long long)(t >> 32);
        kind = pacx_ix_kind((uint32_t)t);
        e = pacx_ix_pos((uint32_t)t);
        at = (g * PACX_IX_GROUP + (long long)((t >> 16) & 0xFFFFu)) * PACX_IX_SEG + e;
        if (kind == PACX_IX_EXIT)
            at += PACX_IX_SEG;                                       /* in the segment after that one */
    }
    const PacxIxResult r = pacx_ix_finish(base, kind, at, n_channels, final, max_records);
    fin[0] = r.n_records;
    fin[1] = r.consumed;
    fin[2] = r.error_at;
}

/* phase 2c, lane g: entry offset (-1: not on the chain) and first record number of the group's segments */
PACX_IX_HD void pacx_ix_fill_group(const uint32_t *tab, long long n_seg, long long g, int32_t gentry, long long gbase,
                                   int32_t *entry, long long *base)
{
    int32_t e = gentry;
    long long b = gbase;
    for (int k = 0; k < PACX_IX_GROUP; ++k) {
        const long long s = g * PACX_IX_GROUP + k;
        if (s >= n_seg)
            continue;
        entry[s] = e;
        base[s] = b;
        if (e < 0)
            continue;
        const uint32_t node = tab[s * PACX_IX_ENTRIES + (e < PACX_IX_ENTRIES ? e : PACX_IX_ENTRIES - 1)];
        b += pacx_ix_count(node);
        e = pacx_ix_kind(node) == PACX_IX_EXIT ? (int32_t)pacx_ix_pos(node) : -1;
    }
}

/* phase 3, lane s: the records that start in segment s, numbered from base; records below n_out are
   written; the lane that meets record number n_out (the first one not returned) writes its prefix's
   position to *consumed when the stitch left that open (fin[1] < 0) */
PACX_IX_HD void pacx_ix_emit_segment(const uint8_t *body, long long n_body, long long s, int32_t entry, long long base,
                                     long long n_out, int need_consumed, long long *offsets, int32_t *n_bytes,
                                     long long *consumed)
{
    if (entry < 0 || entry >= PACX_IX_ENTRIES)
        return;
    int p = entry;
    for (int i = 0; i < PACX_IX_MAX_CHAIN; ++i) {
        if (p >= PACX_IX_SEG)
            return;
        const long long g = s * PACX_IX_SEG + p;
        const uint32_t len = g + 4 <= n_body ? pacx_ix_le32(body + g) : 0u;
        const uint32_t node = pacx_ix_node(p, g, n_body, len);
        const uint32_t kind = pacx_ix_kind(node);
        if (kind != PACX_IX_JUMP && kind != PACX_IX_EXIT)
            return;                                        /* the terminal: the stitch has reported it */
        const long long r = base + i;
        if (r >= n_out) {
            if (r == n_out && need_consumed)
                *consumed = g;
            return;
        }
        offsets[r] = g + 4;
        n_bytes[r] = (int32_t)len;
        p += 4 + (int)len;
    }
}

#endif
