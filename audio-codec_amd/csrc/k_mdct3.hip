/*
 * k_mdct3.hip -- k_mdct_long_v2 with TWO channel-frames in flight per wave
 * (sine window, no per-frame flags: the headline batch).  Same arithmetic, frame
 * by frame, as k_mdct2.hip (both call mdct_dev.h); what changes is the instruction stream: the stages of
 * frames A and B are interleaved, so one frame's LDS round trips hide behind the
 * other's arithmetic, and every table value read from LDS (window, pre/post
 * twiddle, per-lane FFT twiddles) serves both frames.  LDS: one 8 KB FFT tile and
 * two 4 KB PCM landing buffers per wave + the 24 KB of tables.
 */
#include "pacx_launch.h"
#include "mdct_dev.h"

/*
 * k_mdct_long_x2p: the two frames of a wave take turns on ONE 8 KB FFT tile, exchange
 * by exchange (A writes, B computes, A reads back, B writes, ...), which leaves 8 KB per
 * wave for two PCM landing buffers of their own.  The next pair's LDS-DMA is then
 * issued right after the fold -- it has the whole FFT and epilogue to arrive instead of
 * the epilogue only -- and, being older than the epilogue's stores, is waited for with
 * a counted vmcnt that leaves those stores in flight.  A frame's reads of the tile are
 * followed by the other frame's writes without a wait in between: the DS instructions
 * of one wave execute in issue order.  The DMA is issued from inline assembly, so
 * the compiler's waitcnt pass does not know of it: it would otherwise put a
 * conservative vmcnt(0) before the next LDS read (it cannot tell the landing buffers
 * from the tile), which is what kept the landing-buffer variant of k_mdct2.hip from
 * prefetching.
 */
/* M0 (the DMA's LDS base) is on the asm's clobber list: the compiler sets M0 right before
   each of its own uses and keeps nothing live in it, the list entry only says so */
#pragma clang diagnostic push
#pragma clang diagnostic ignored "-Winline-asm"
#ifdef PACX_MDCT_DEBUG
__device__ long long g_mdct_dbg[8 * 16];
#define DBG_T(k) do { long long t_; asm volatile("s_waitcnt lgkmcnt(0)\n\ts_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_) :: "memory"); \
                      if (dbg_on) dbg_acc[k] += t_ - dbg_last; dbg_last = t_; } while (0)
extern "C" int pacx_debug_read(long long *out, int n)
{
    return (int)hipMemcpyFromSymbol(out, HIP_SYMBOL(g_mdct_dbg), sizeof(long long) * n);
}
#else
#define DBG_T(k) do { } while (0)
#endif
/* STEP: the instantiation the whole-path entry points launch (it also initialises the frames' status words and
   sub-block scales); the stand-alone pacx_mdct_batch launches STEP = false.  Two symbols, so that a kernel trace
   tells the stand-alone launches -- the ones the HBM roofline figure is quoted on -- from the in-step ones, which
   run beside the side chain and, with two steps in flight, beside another step's kernels, and are stretched by it */
template <int WAVES, int MINW, bool STEP>
__global__ __launch_bounds__(64 * WAVES, MINW) void k_mdct_long_x2p(PacxTables T, PacxPcmView in, long long n_cf,
                                                                   double *__restrict__ lines,
                                                                   int32_t *__restrict__ scale_out,
                                                                   int scale_stride,
                                                                   uint32_t *__restrict__ status_init)
{
    __shared__ __attribute__((aligned(16))) cplx tiles[WAVES][WFFT_TILE_N];
    __shared__ __attribute__((aligned(16))) short raws[WAVES][2][PACX_N_LONG];
    __shared__ __attribute__((aligned(16))) MdctLongTables tb;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
    cplx *tile = tiles[wv];
    const unsigned n_ch = (unsigned)in.n_ch;
    const unsigned n_waves = gridDim.x * WAVES;
    const unsigned total = (unsigned)n_cf;
    const short *base = (const short *)in.base;
    auto stage = [&](unsigned c, int f) {
        const unsigned fr = c / n_ch, ch = c - fr * n_ch;
        const int4 *src = (const int4 *)(base + (long long)fr * in.frame_stride + (long long)ch * in.ch_stride);
        const unsigned lds = __builtin_amdgcn_readfirstlane(
            (unsigned)(size_t)(__attribute__((address_space(3))) char *)(char *)raws[wv][f]);
        asm volatile("s_mov_b32 m0, %1\n\ts_nop 0\n\t"
                     "global_load_lds_dwordx4 %0, off\n\t"
                     "global_load_lds_dwordx4 %0, off offset:1024\n\t"
                     "global_load_lds_dwordx4 %0, off offset:2048\n\t"
                     "global_load_lds_dwordx4 %0, off offset:3072"
                     :: "v"(src + lane), "s"(lds) : "memory", "m0");
    };
    const unsigned vb = pacx_xcd_block(blockIdx.x, gridDim.x);    /* XCD-aware frame order (pacx_dev.h) */
    const unsigned g = vb * WAVES + wv;
    unsigned cfa = g, cfb = g + n_waves;
    if (cfa < total)
        stage(cfa, 0);
    if (cfb < total)
        stage(cfb, 1);
    tb.stage<64 * WAVES>(T, tid);
    __syncthreads();

    const cplx *w1 = tb.w1(lane), *w2 = tb.w2(lane);
    auto epilogue = [&](const cplx *v, unsigned cf) {
        mdct_long_epilogue(T, v, [&](int k3) { return tb.twl[lane + 64 * k3]; }, cf, lane, lines, scale_out,
                           scale_stride, STEP ? status_init : nullptr);
    };
#ifdef PACX_MDCT_DEBUG
    const bool dbg_on = blockIdx.x == 7;
    long long dbg_acc[8] = {0, 0, 0, 0, 0, 0, 0, 0}, dbg_last = 0;
    DBG_T(7);
    dbg_acc[7] = 0;
#endif
    bool first = true;
    for (; cfa < total; cfa += 2 * n_waves, cfb += 2 * n_waves) {
        const bool has_b = cfb < total;
        /* this pair's PCM must have landed; what was issued after its DMA -- the previous
           pair's 16 line stores (and 2 scale stores) -- may stay in flight.  Vector memory
           operations complete in issue order, so a count that is not above the number of
           younger operations is safe, a smaller one merely waits for more */
        if (first)
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        else
            asm volatile("s_waitcnt vmcnt(%0)" :: "n"(2 * EPI_STORES) : "memory");   /* the two epilogues' line
                                       stores; the 2 scale stores, when there are any, only make the wait stricter */
        first = false;
        DBG_T(0);
        wave_lds_fence();
        cplx v[2][8];
        for (int pass = 0;; ++pass) {
            int lowest[2] = {0, 0};
#pragma unroll
            for (int n1 = 0; n1 < 8; ++n1) {
                const int n = lane + 64 * n1;
                int i0, i1, i2, i3, ia, ib;
                mdct_fold_index<PACX_N_LONG>(n1, n, i0, i1, i2, i3);
                mdct_fold_sym_index(n1, i0, i1, i2, i3, ia, ib);
                const double wa = tb.wsin[ia], wb = tb.wsin[ib];     /* every table value serves both frames */
                const cplx tw = tb.twl[n];
#pragma unroll
                for (int f = 0; f < 2; ++f) {
                    double c0, c1, c2, c3;
                    mdct_fold_codes<true>(raws[wv][f], i0, i1, i2, i3, c0, c1, c2, c3, lowest[f]);
                    v[f][n1] = c_mul(mdct_fold_sym(n1, wa, wb, c0, c1, c2, c3), tw);
                }
            }
            if (pass || !__builtin_amdgcn_ballot_w64(lowest[0] == -32768 || lowest[1] == -32768))
                break;
            wave_lds_fence();
#pragma unroll
            for (int f = 0; f < 2; ++f)
                mdct_zero_min_codes((unsigned *)raws[wv][f], lane);
            wave_lds_fence();
        }
        wave_lds_fence();
        /* the landing buffers are consumed (the DMA is not ordered with this wave's own
           ds_reads: they must have returned): next pair's PCM on its way.  The output
           initialisation goes first so that it is older than the DMA. */
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        DBG_T(1);
        if (STEP && status_init) {
            if (lane == 0) {
                status_init[cfa] = 0u;
                if (has_b)
                    status_init[cfb] = 0u;
            }
            if (lane >= 1 && lane < PACX_SUB) {
                scale_out[(long long)cfa * PACX_SUB + lane] = 0;
                if (has_b)
                    scale_out[(long long)cfb * PACX_SUB + lane] = 0;
            }
        }
        if (cfa + 2 * n_waves < total)
            stage(cfa + 2 * n_waves, 0);
        if (cfb + 2 * n_waves < total)
            stage(cfb + 2 * n_waves, 1);
        DBG_T(2);

        /* 512-point FFTs (wave_fft.h fft512n), the two frames alternating on the tile */
        dft8(v[0]); fft512n_twiddle(v[0], w1, 64); fft512n_x1_write(tile, v[0], lane);
        dft8(v[1]); fft512n_twiddle(v[1], w1, 64);
        wave_lds_fence(); fft512n_x1_read(tile, v[0], lane); fft512n_x1_write(tile, v[1], lane);
        dft8(v[0]); fft512n_twiddle(v[0], w2, 8);
        wave_lds_fence(); fft512n_x1_read(tile, v[1], lane); fft512n_x2_write(tile, v[0], lane);
        dft8(v[1]); fft512n_twiddle(v[1], w2, 8);
        wave_lds_fence(); fft512n_x2_read(tile, v[0], lane); fft512n_x2_write(tile, v[1], lane);
        dft8(v[0]);
        wave_lds_fence(); fft512n_x2_read(tile, v[1], lane);
        DBG_T(3);
        epilogue(v[0], cfa);
        DBG_T(4);
        dft8(v[1]);
        if (has_b)
            epilogue(v[1], cfb);
        wave_lds_fence();
        DBG_T(5);
    }
#ifdef PACX_MDCT_DEBUG
    if (dbg_on && lane == 0)
        for (int k = 0; k < 8; ++k)
            g_mdct_dbg[wv * 16 + k] = dbg_acc[k];
#endif
}

#pragma clang diagnostic pop

void pacx_k::pacx_launch_mdct_x2(const PacxTables &T, const PacxPcmView &in, long long n_cf, double *lines,
                         int32_t *scale_out, int scale_stride, uint32_t *status_init, int n_cu, hipStream_t st)
{
    long long blocks = (n_cf + 2 * 8 - 1) / (2 * 8);
    if (blocks > n_cu)
        blocks = n_cu;
    if (status_init)
        hipLaunchKernelGGL((k_mdct_long_x2p<8, 2, true>), dim3((unsigned)blocks), dim3(64 * 8), 0, st, T, in, n_cf, lines,
                           scale_out, scale_stride, status_init);
    else
        hipLaunchKernelGGL((k_mdct_long_x2p<8, 2, false>), dim3((unsigned)blocks), dim3(64 * 8), 0, st, T, in, n_cf, lines,
                           scale_out, scale_stride, status_init);
}
