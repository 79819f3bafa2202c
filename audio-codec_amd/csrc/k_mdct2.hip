/*
 * k_mdct2.hip -- the roofline kernel: window + MDCT of long blocks, int16 PCM in
 * (unit stride, 16-byte aligned rows), float64 lines out.  Same math as
 * k_mdct.hip (reference: coder/window.py:14-25, coder/mdct.py:43-69 at
 * coder/codec.py:303-311) laid out for throughput; the arithmetic of a frame is
 * mdct_dev.h's, this file holds the staging and the loop over frames:
 *
 *   - persistent workgroups of 8 waves, one channel-frame per wave at a time,
 *     grid-stride over frames; twiddle table d[n] and the sine window live in
 *     LDS once per workgroup, the per-lane FFT twiddles in registers;
 *   - the next frame's 4 KB of PCM is prefetched into registers (4 x 16-byte
 *     coalesced loads per lane) while the current frame is transformed;
 *   - natural-order 512-point FFT (wave_fft.h fft512n) on an 8 KB swizzled tile
 *     that also stages the raw int16 samples, so LDS is 8 KB per wave;
 *   - lane L ends up holding y[L + 64 j]; X[2k] = Re y[k] and
 *     X[2k+1] = -Im y[511-k] sit in mirrored lanes, one 64-lane reversal
 *     (ds_bpermute) pairs them so every store is a contiguous 16 bytes per lane
 *     (1 KB per wave instruction).
 *
 * HBM traffic per channel-frame: 2 KB of new PCM (the other half of the window
 * was read by the previous frame and is an L2 hit) + 8 KB of lines = 10 240 B.
 */
#include "pacx_launch.h"
#include "mdct_dev.h"

/* 8 waves per workgroup (8 KB tile each + 24 KB of tables + 48 KB of transition windows),
   one workgroup per CU, two waves per SIMD */
#define MDCT2_WAVES 8
__global__ __launch_bounds__(64 * MDCT2_WAVES, 2) void k_mdct_long_v2(
    PacxTables T, PacxPcmView in, const uint8_t *__restrict__ flags, long long n_cf, int skip_cur,
    double *__restrict__ lines, int32_t *__restrict__ scale_out, int scale_stride,
    uint32_t *__restrict__ status_init, const int32_t *__restrict__ cf_list,
    const int32_t *__restrict__ cf_count)
{
    __shared__ __attribute__((aligned(16))) cplx tiles[MDCT2_WAVES][WFFT_TILE_N];
    __shared__ __attribute__((aligned(16))) MdctLongTables tb;
    /* the three transition windows (start / stop / start-stop, coder/window.py:61-92),
       scaled like tb.wsin, whole: a frame's window kind is wave-uniform, so a fold element reads
       its four values at plain per-lane indices -- no region tests, no global loads whose 32
       results in flight per frame had the kernel at 256 registers with 23 spilled */
    __shared__ __attribute__((aligned(16))) double wtr[3][PACX_N_LONG];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);     /* wave-uniform: frame index math on the SALU */
    cplx *tile = tiles[wv];
    short *raw = (short *)tile;            /* the raw int16 samples are staged in the FFT tile */
    const unsigned n_ch = (unsigned)in.n_ch;
    const unsigned stride = gridDim.x * MDCT2_WAVES;
    /* mixed streams: walk the compacted list of the long-coded frames (k_frame_lists) instead
       of every frame -- on a castanet stream half of the frames are short-coded, and staging
       their PCM only to skip them was half of this kernel's time */
    const unsigned total = cf_list ? (unsigned)*cf_count : (unsigned)n_cf;
    auto frame_of = [&](unsigned i) -> unsigned { return cf_list ? (unsigned)cf_list[i] : i; };
    const short *base = (const short *)in.base;
    /* PCM goes HBM -> LDS without touching VGPRs (global_load_lds_dwordx4:
       wave-uniform LDS base + lane*16, per-lane global address) */
    auto stage = [&](unsigned c) {
        const unsigned f = c / n_ch, ch = c - f * n_ch;
        const int4 *src = (const int4 *)(base + (long long)f * in.frame_stride + (long long)ch * in.ch_stride);
#pragma unroll
        for (int j = 0; j < 4; ++j)
            __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void *)(src + lane + 64 * j),
                                             (__attribute__((address_space(3))) void *)((char *)raw + 1024 * j),
                                             16, 0, 0);
    };
    const unsigned vb = pacx_xcd_block(blockIdx.x, gridDim.x);    /* XCD-aware frame order (pacx_dev.h) */
    unsigned it = vb * MDCT2_WAVES + wv;              /* position in the list (or the frame itself) */
    unsigned cf_next = it < total ? frame_of(it) : 0u;
    if (it < total)
        stage(cf_next);               /* first frame's PCM flies while the tables load */
    tb.stage<64 * MDCT2_WAVES>(T, tid);
    for (int i = tid; i < 3 * PACX_N_LONG; i += 64 * MDCT2_WAVES)
        wtr[0][i] = T.win_long[PACX_N_LONG + i] * MDCT_LONG_KSCALE;
    __syncthreads();

    for (; it < total; it += stride) {
        const unsigned cf = cf_next;
        if (it + stride < total)
            cf_next = frame_of(it + stride);          /* read one iteration ahead of its DMA */
        const unsigned fl = flags ? flags[cf / n_ch] : 0u;
        /* frames this kernel leaves to k_mdct_short: short-coded (CUR) ones when asked to */
        const bool mine = !(skip_cur && (fl & 2u));
        /* transition windows (start / stop / start-stop) are not symmetric: their four
           values per fold element come from the LDS tables wtr */
        const int kind = __builtin_amdgcn_readfirstlane(pacx_window_kind(fl));
        const double *gw = wtr[kind > 0 ? kind - 1 : 0];
        /* output initialisation the whole-path entry points would otherwise spend two
           memset launches on: status word 0 and the 7 unused overall-scale slots of a
           long frame 0, for EVERY frame (kernels that follow on the stream overwrite /
           OR into them for the frames they own) */
        if (status_init) {
            if (lane == 0)
                status_init[cf] = 0u;
            if (lane >= 1 && lane < PACX_SUB)
                scale_out[(long long)cf * PACX_SUB + lane] = 0;
        }
        /* this frame's PCM must have landed in LDS (the DMA is the youngest vector-memory
           operation but for the two initialisation stores above: wait for everything) */
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        wave_lds_fence();
        if (!mine) {
            /* a short-coded frame (k_mdct_short's): nothing to transform, only the chain of
               PCM fetches to keep going -- on a castanet stream that is more than half of
               the frames */
            if (it + stride < total)
                stage(cf_next);
            continue;
        }
        cplx v[8];
        /* the second pass is rare: one copy of the fold per window form, not one per pass as well */
#pragma nounroll
        for (int pass = 0;; ++pass) {
            int lowest = 0;
#pragma unroll
            for (int n1 = 0; n1 < 8; ++n1) {
                const int n = lane + 64 * n1;
                int i0, i1, i2, i3, ia, ib;
                mdct_fold_index<PACX_N_LONG>(n1, n, i0, i1, i2, i3);
                mdct_fold_sym_index(n1, i0, i1, i2, i3, ia, ib);
                /* window values before the codes: with the code loads ahead of them the compiler
                   kept 11 registers of this kernel in scratch */
                double c0, c1, c2, c3;
                cplx u;
                if (kind == 0) {
                    const double wa = tb.wsin[ia], wb = tb.wsin[ib];
                    mdct_fold_codes<true>(raw, i0, i1, i2, i3, c0, c1, c2, c3, lowest);
                    u = mdct_fold_sym(n1, wa, wb, c0, c1, c2, c3);
                } else {
                    const double w0 = gw[i0], w1 = gw[i1], w2 = gw[i2], w3 = gw[i3];
                    mdct_fold_codes<true>(raw, i0, i1, i2, i3, c0, c1, c2, c3, lowest);
                    u = mdct_fold_any(n1, w0, w1, w2, w3, c0, c1, c2, c3);
                }
                v[n1] = c_mul(u, tb.twl[n]);
            }
            if (pass || !__builtin_amdgcn_ballot_w64(lowest == -32768))
                break;
            wave_lds_fence();
            mdct_zero_min_codes((unsigned *)raw, lane);
            wave_lds_fence();
        }
        wave_lds_fence();                 /* raw samples consumed: their LDS may be overwritten */
        fft512n(v, tile, tb.w1(lane), 64, tb.w2(lane), 8, lane);
        /* the tile is free again: start the next frame's PCM on its way now, it
           lands during the epilogue and the other waves' work.  The DMA writes
           LDS from the vector-memory side and is not ordered with this wave's
           own ds_reads, so the FFT's last tile reads must have returned first
           (a wavefront-scope fence does not wait for them; hazard table in DESIGN.md,
           checked on the compiled code by tests/test_build_isa.py). */
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        if (it + stride < total)
            stage(cf_next);
        mdct_long_epilogue(T, v, [&](int k3) { return tb.twl[lane + 64 * k3]; }, cf, lane, lines, scale_out,
                           scale_stride, status_init);
    }
}

void pacx_k::pacx_launch_mdct_v2(const PacxTables &T, const PacxPcmView &in, const uint8_t *flags, long long n_cf,
                         int skip_cur, double *lines, int32_t *scale_out, int scale_stride,
                         uint32_t *status_init, int n_cu, const int32_t *cf_list, const int32_t *cf_count,
                         hipStream_t st)
{
    if (n_cf <= 0)
        return;
    if (status_init && (!scale_out || scale_stride != PACX_SUB))
        status_init = nullptr;                 /* the caller keeps its memsets */
    /* batches without per-frame flags (all sine windows) go to the pipelined two-frames-per-wave kernel of
       k_mdct3.hip; batches with flags (transition windows, frames left to the short kernel) stay here */
    if (!flags) {
        pacx_launch_mdct_x2(T, in, n_cf, lines, scale_out, scale_stride, status_init, n_cu, st);
        return;
    }
    long long blocks = (n_cf + MDCT2_WAVES - 1) / MDCT2_WAVES;
    if (blocks > n_cu)
        blocks = n_cu;                         /* one persistent workgroup per CU */
    hipLaunchKernelGGL(k_mdct_long_v2, dim3((unsigned)blocks), dim3(64 * MDCT2_WAVES), 0, st, T, in,
                       flags, n_cf, skip_cur, lines, scale_out, scale_stride, status_init, cf_list, cf_count);
}
