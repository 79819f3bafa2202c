/*
 * k_index.hip -- record index of a .pac body on the device (pacx_index_body, include/pacx.h).
 *
 * The phases and the encoding of their tables are body_index.h's; this file holds the one phase that
 * needs a workgroup (the segment maps: pointer jumping in LDS) and the thin kernels that give the
 * other phases their lanes.  Every loop below has a trip count fixed by PACX_IX_SEG, PACX_IX_ENTRIES,
 * PACX_IX_GROUP or the number of segments / groups: a body built to defeat the scheme (one-byte
 * records, prefixes everywhere) costs the same time as any other, never a hang.
 */
#include "body_index.h"
#include "pacx_launch.h"

/* body_index.h is also compiled on its own (the CPU model of the index), so it names the bound itself */
static_assert(PACX_IX_MAX_RECORD == PACX_PAYLOAD_STRIDE, "a record is at most one payload slot");

#define IX_THREADS 256

/* phase 1: one workgroup per segment.  LDS: the segment's bytes (+3 of look-ahead) and two buffers of
   nodes (a round reads one and writes the other: the record counts are not idempotent) = 72 KB, two
   workgroups per CU. */
__global__ __launch_bounds__(IX_THREADS) void k_index_segments(const uint8_t *__restrict__ body, long long n_body,
                                                               uint32_t *__restrict__ tab)
{
    __shared__ uint8_t by[PACX_IX_SEG + 4];
    __shared__ uint32_t nd[2][PACX_IX_SEG];
    const long long seg0 = (long long)blockIdx.x * PACX_IX_SEG;
    for (int i = threadIdx.x; i < PACX_IX_SEG + 4; i += IX_THREADS) {
        const long long g = seg0 + i;
        by[i] = g < n_body ? body[g] : (uint8_t)0;
    }
    __syncthreads();
    for (int p = threadIdx.x; p < PACX_IX_SEG; p += IX_THREADS)
        nd[0][p] = pacx_ix_node(p, seg0 + p, n_body, pacx_ix_le32(by + p));
    __syncthreads();
    int cur = 0;
    for (int r = 0; r < PACX_IX_ROUNDS; ++r) {
        for (int p = threadIdx.x; p < PACX_IX_SEG; p += IX_THREADS) {
            uint32_t a = nd[cur][p];
            if (pacx_ix_kind(a) == PACX_IX_JUMP)
                a = pacx_ix_jump(a, nd[cur][pacx_ix_pos(a)]);        /* pos < PACX_IX_SEG by its 13 bits */
            nd[cur ^ 1][p] = a;
        }
        __syncthreads();
        cur ^= 1;
    }
    uint32_t *__restrict__ out = tab + (long long)blockIdx.x * PACX_IX_ENTRIES;
    for (int e = threadIdx.x; e < PACX_IX_ENTRIES; e += IX_THREADS)
        out[e] = nd[cur][e];
}

/* phase 2a: lane (group, entry offset) */
__global__ __launch_bounds__(IX_THREADS) void k_index_compose(const uint32_t *__restrict__ tab, long long n_seg,
                                                              uint64_t *__restrict__ gtab)
{
    const int e = blockIdx.x * IX_THREADS + threadIdx.x;
    const long long g = blockIdx.y;
    if (e < PACX_IX_ENTRIES)
        gtab[g * PACX_IX_ENTRIES + e] = pacx_ix_compose_lane(tab, n_seg, g, e);
}

/* phase 2b: one lane, one dependent load per group */
__global__ void k_index_stitch(const uint64_t *__restrict__ gtab, long long n_groups, int n_ch, int final,
                               long long max_records, int32_t *__restrict__ gentry, long long *__restrict__ gbase,
                               long long *__restrict__ fin, long long *__restrict__ result)
{
    if (blockIdx.x != 0 || threadIdx.x != 0)
        return;
    long long f[3];
    pacx_ix_stitch(gtab, n_groups, n_ch, final, max_records, gentry, gbase, f);
    fin[0] = f[0];
    fin[1] = f[1];
    fin[2] = f[2];
    result[0] = f[0];
    if (f[1] >= 0)
        result[1] = f[1];                       /* otherwise the lane of k_index_emit that meets record f[0] */
    result[2] = f[2];
}

/* phase 2c: lane per group */
__global__ __launch_bounds__(64) void k_index_fill(const uint32_t *__restrict__ tab, long long n_seg, long long n_groups,
                                                   const int32_t *__restrict__ gentry, const long long *__restrict__ gbase,
                                                   int32_t *__restrict__ entry, long long *__restrict__ base)
{
    const long long g = (long long)blockIdx.x * 64 + threadIdx.x;
    if (g < n_groups)
        pacx_ix_fill_group(tab, n_seg, g, gentry[g], gbase[g], entry, base);
}

/* phase 3: lane per segment */
__global__ __launch_bounds__(64) void k_index_emit(const uint8_t *__restrict__ body, long long n_body, long long n_seg,
                                                   const int32_t *__restrict__ entry, const long long *__restrict__ base,
                                                   const long long *__restrict__ fin, long long *__restrict__ offsets,
                                                   int32_t *__restrict__ n_bytes, long long *__restrict__ result)
{
    const long long s = (long long)blockIdx.x * 64 + threadIdx.x;
    if (s < n_seg)
        pacx_ix_emit_segment(body, n_body, s, entry[s], base[s], fin[0], fin[1] < 0, offsets, n_bytes, result + 1);
}

size_t pacx_k::pacx_index_ws_bytes(long long n_body, PacxIndexWs *ws)
{
    const long long n_seg = pacx_ix_segments(n_body), n_groups = pacx_ix_groups(n_seg);
    size_t at = 0;
    auto take = [&at](size_t bytes) { const size_t o = at; at += (bytes + 255) & ~(size_t)255; return o; };
    ws->n_seg = n_seg;
    ws->n_groups = n_groups;
    ws->gtab = take((size_t)n_groups * PACX_IX_ENTRIES * sizeof(uint64_t));
    ws->gbase = take((size_t)n_groups * sizeof(long long));
    ws->base = take((size_t)n_seg * sizeof(long long));
    ws->fin = take(3 * sizeof(long long));
    ws->tab = take((size_t)n_seg * PACX_IX_ENTRIES * sizeof(uint32_t));
    ws->gentry = take((size_t)n_groups * sizeof(int32_t));
    ws->entry = take((size_t)n_seg * sizeof(int32_t));
    return at;
}

void pacx_k::pacx_launch_index(const PacxIndexWs &ws, char *mem, const uint8_t *body, long long n_body, int n_ch, int final,
                       long long max_records, long long *offsets, int32_t *n_bytes, long long *result, hipStream_t st)
{
    uint32_t *tab = (uint32_t *)(mem + ws.tab);
    uint64_t *gtab = (uint64_t *)(mem + ws.gtab);
    int32_t *gentry = (int32_t *)(mem + ws.gentry), *entry = (int32_t *)(mem + ws.entry);
    long long *gbase = (long long *)(mem + ws.gbase), *base = (long long *)(mem + ws.base), *fin = (long long *)(mem + ws.fin);
    hipLaunchKernelGGL(k_index_segments, dim3((unsigned)ws.n_seg), dim3(IX_THREADS), 0, st, body, n_body, tab);
    hipLaunchKernelGGL(k_index_compose, dim3((PACX_IX_ENTRIES + IX_THREADS - 1) / IX_THREADS, (unsigned)ws.n_groups),
                       dim3(IX_THREADS), 0, st, tab, ws.n_seg, gtab);
    hipLaunchKernelGGL(k_index_stitch, dim3(1), dim3(1), 0, st, gtab, ws.n_groups, n_ch, final, max_records, gentry, gbase,
                       fin, result);
    hipLaunchKernelGGL(k_index_fill, dim3((unsigned)((ws.n_groups + 63) / 64)), dim3(64), 0, st, tab, ws.n_seg, ws.n_groups,
                       gentry, gbase, entry, base);
    hipLaunchKernelGGL(k_index_emit, dim3((unsigned)((ws.n_seg + 63) / 64)), dim3(64), 0, st, body, n_body, ws.n_seg, entry,
                       base, fin, offsets, n_bytes, result);
}
