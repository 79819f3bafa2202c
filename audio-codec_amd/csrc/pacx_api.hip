/*
 * pacx_api.hip -- the C ABI of include/pacx.h: handle, resident tables,
 * grow-only workspace, argument checking, kernel sequencing on a HIP stream.
 */
#include <hip/hip_runtime.h>

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <cmath>
#include <string>
#include <vector>

#include "../../include/pacx.h"
#include "body_index.h"
#include "pacx_launch.h"
#include "pvq_dev.h"
#include "pacx_vq_tables.h"
#include "pacx_tables_gen.h"

using namespace pacx_k;

/* Path overrides.  Each forces a path that runs by default on some other input, so that the GPU tests can hold
   the two implementations bit-identical on one batch.  Read once, when the handle is created; -1 (unset, or a
   value the variable does not take): the default. */
struct PacxOverrides {
    int split_short;                  /* PACX_SPLIT_SHORT=0: block-switched batches on one stream */
    int fuse_tail;                    /* PACX_FUSE_TAIL=0/1: the long frames' tail in k_tail_long / in k_mask */
    int fuse_front;                   /* PACX_FUSE_FRONT=0/1: all-long steps' MDCT in k_mdct_long_x2p / in k_front_long */
    int vq_fuse_alloc;                /* PACX_VQ_FUSE_ALLOC=0/1: the long frames' BitAlloc in k_bitalloc / in k_mask */
    int vq_frame;                     /* PACX_VQ_FRAME=0: k_vq over every unit */
    int vq_bfs;                       /* PACX_VQ_BFS=n: level walk from n shape bits (0: depth first only) */
    int vq_dec_frame;                 /* PACX_VQ_DEC_FRAME=0: k_vq_dec over every block */
};

#define PACX_FUSE_FRONT_DEFAULT 1     /* follows the measurement of DESIGN.md 5.4 */

/* an integer in [lo, hi] from the environment, else -1 */
static int env_override(const char *name, int lo, int hi)
{
    const char *e = getenv(name);
    if (!e || !*e)
        return -1;
    char *end;
    const long v = strtol(e, &end, 10);
    return (*end || v < lo || v > hi) ? -1 : (int)v;
}

static PacxOverrides read_overrides(void)
{
    PacxOverrides o;
    o.split_short = env_override("PACX_SPLIT_SHORT", 0, 0);
    o.fuse_tail = env_override("PACX_FUSE_TAIL", 0, 1);
    o.fuse_front = env_override("PACX_FUSE_FRONT", 0, 1);
    o.vq_fuse_alloc = env_override("PACX_VQ_FUSE_ALLOC", 0, 1);
    o.vq_frame = env_override("PACX_VQ_FRAME", 0, 0);
    o.vq_bfs = env_override("PACX_VQ_BFS", 0, 1 << 20);
    o.vq_dec_frame = env_override("PACX_VQ_DEC_FRAME", 0, 0);
    return o;
}

struct pacx_handle {
    int device;
    int n_cu;                         /* compute units (persistent-kernel grid sizing) */
    PacxOverrides force;
    PacxTables T;
    std::vector<void *> owned;        /* table allocations                      */
    /* workspace (device), sized for ws_cf channel-frames */
    long long ws_cf;
    double *ws_lines;                 /* [ws_cf][1024]                          */
    double *ws_smr;                   /* [ws_cf][band_stride]                   */
    PacxPeak *ws_peaks;               /* [ws_cf][512]                           */
    int32_t *ws_npeaks;               /* [ws_cf][8] maskers found               */
    int32_t *ws_nkept;                /* [ws_cf][8] maskers left after pruning  */
    int32_t *ws_overall;              /* [ws_cf][8]                             */
    long long *ws_chunks;             /* [ws_cf/256 + 2]                        */
    long long *ws_offs;               /* [ws_cf]                                */
    int32_t *ws_lists;                /* [2*ws_cf + 2] long cf list, short cf list, counts */
    long long ws_blocks_cf;           /* decode: capacity of ws_blocks          */
    double *ws_blocks;                /* [cf][2048] blocks before overlap-add   */
    /* gain-shape coder (use_vq) */
    /* fork-join: the side chain (VALU/latency bound) runs beside the MDCT (HBM bound) */
    int fork_side;                    /* all-long scalar batches: side chain on side_stream (pacx_set_side_fork) */
    hipStream_t side_stream;
    hipEvent_t ev_fork, ev_join;
    /* mixed batches: the short-coded frames' chain (MDCT, side chain, mask, tail) runs on
       a stream of its own beside the long-coded frames' */
    hipStream_t short_stream;
    hipStream_t spare_stream;         /* unused: keeps HIP's queue map of later streams (without it bs128 32.5 vs 34.9 M cf/s) */
    hipEvent_t ev_short_done, ev_lists;
    std::vector<char> vq_view;        /* VqView of k_vq.hip (device pointers)   */
    std::vector<char> vqdec_view;     /* VqDecView of k_vq_dec.hip              */
    int tables_exact;                 /* every float64 table is the NumPy-evaluated one */
    long long ws_mant_cf;             /* capacity of ws_mant                    */
    int32_t *ws_mant;                 /* [cf][1024] mantissas of short frames when the caller wants none */
    long long ws_dec_cf;              /* capacity of the VQ decode buffers      */
    double *ws_dec_lines;             /* [cf][1024]                             */
    uint8_t *ws_dec_sbr;              /* [cf]                                   */
    uint32_t *ws_dec_status;          /* [cf] (scalar SBR decode without a caller's status) */
    double *ws_sbr_mean;              /* [ws_cf][8] omitted-band means           */
    long long ws_vq_cf;               /* capacity of the short-frame buffers    */
    unsigned *ws_unit_words;          /* [ws_vq_cf*8][PACX_PAYLOAD_WORDS]       */
    int32_t *ws_unit_bits;            /* [ws_vq_cf*8][2]                        */
    long long ws_index_bytes;         /* capacity of ws_index                   */
    char *ws_index;                   /* pacx_index_body's tables (PacxIndexWs)  */
    long long ws_thr_cf;              /* capacity of ws_thr (0 until the first pacx_nmr_batch) */
    double *ws_thr;                   /* [cf][1024] masked threshold, dB SPL     */
    uint32_t *ws_rate_status;         /* [cf] status words of pacx_rate_curve_batch's front end (capacity ws_thr_cf) */
    long long ws_solve_n;             /* states ws_solve holds: 1 for the plain solves, n_seg for the segmented, n_seg + 1
                                         for the peak solves (the stream's state behind the segments') */
    char *ws_solve;                   /* [ws_solve_n] the solve's state per segment */
    long long *ws_seg;                /* [3 ws_solve_n] a solve's boundaries [n_seg + 1], then its limits [n_seg]: uploaded by
                                         the segmented solves, written by the init kernel for the plain ones */
    char *ws_bucket;                  /* the one state of a buffered solve (k_bucket.hip), whatever ws_solve_n */
    char *ws_pin;                     /* a pinned solve's state, F_h and pins (k_bucket_pin.hip): ws_solve_n hops */
    long long seg_host_n;             /* segments the pinned staging copy holds  */
    long long *seg_host;              /* [2 seg_host_n + 1] pinned: what ws_seg is uploaded from */
    hipEvent_t ev_seg;                /* the last upload from seg_host           */
    long long ws_vqb_cf;              /* capacity of ws_vqb (0 until the first pacx_vq_band_curve_batch) */
    char *ws_vqb;                     /* one pass of the gain-shape band curve: payload slots, the pass's allocation and
                                         status words, what the decoder reads back, k_nmr's rows (vq_band_ws) */
    std::string err;
};

static thread_local std::string g_create_err;

static int fail(pacx_handle *h, int code, const std::string &msg)
{
    if (h)
        h->err = msg;
    else
        g_create_err = msg;
    return code;
}

#define HIP_TRY(h, call)                                                               \
    do {                                                                               \
        hipError_t e_ = (call);                                                        \
        if (e_ != hipSuccess)                                                          \
            return fail(h, PACX_E_HIP, std::string(#call) + ": " + hipGetErrorString(e_)); \
    } while (0)

/* Inside a fork/join region (work already queued on the handle's internal streams, which share the
   handle's workspaces with the caller's stream): an error must not leave those streams unjoined --
   the caller's next call could overwrite ws_lines / ws_smr / ws_peaks / ws_lists under kernels that
   are still running.  On the error path the internal streams are drained before returning. */
static void drain_internal(pacx_handle *h);
#define HIP_TRY_FORKED(h, call)                                                        \
    do {                                                                               \
        hipError_t e_ = (call);                                                        \
        if (e_ != hipSuccess) {                                                        \
            drain_internal(h);                                                         \
            return fail(h, PACX_E_HIP, std::string(#call) + ": " + hipGetErrorString(e_)); \
        }                                                                              \
    } while (0)

template <typename Tp>
static int upload(pacx_handle *h, const Tp *host, size_t n, const Tp **dev)
{
    void *p = nullptr;
    HIP_TRY(h, hipMalloc(&p, n * sizeof(Tp)));
    h->owned.push_back(p);
    HIP_TRY(h, hipMemcpy(p, host, n * sizeof(Tp), hipMemcpyHostToDevice));
    *dev = (const Tp *)p;
    return PACX_OK;
}

static std::vector<double2> unit_circle(int count, long double num_mul, long double num_add, long double den)
{
    /* exp(-j*pi*(num_mul*i + num_add)/den), evaluated in long double */
    std::vector<double2> t(count);
    const long double pi = 3.14159265358979323846264338327950288L;
    for (int i = 0; i < count; ++i) {
        const long double a = pi * (num_mul * i + num_add) / den;
        t[i].x = (double)cosl(a);
        t[i].y = (double)(-sinl(a));
    }
    return t;
}

/* built-in float64 tables (pacx_tables_gen.h): bit patterns of the NumPy evaluation */
static std::vector<double> gen_table(const uint64_t *bits, size_t n)
{
    std::vector<double> t(n);
    memcpy(t.data(), bits, n * sizeof(double));
    return t;
}

static int gen_rate_index(int sample_rate)
{
    for (int i = 0; i < PACX_GEN_N_RATES; ++i)
        if (PACX_GEN_RATES[i] == sample_rate)
            return i;
    return -1;
}

extern "C" int pacx_tables_exact(const pacx_handle *h) { return h ? h->tables_exact : PACX_E_ARG; }

/* coder/psychoac.py:100-103 */
static const double kCbFreqLimits[25] = {100, 200, 300, 400, 510, 630, 770, 920, 1080, 1270, 1480, 1720, 2000,
                                         2320, 2700, 3150, 3700, 4400, 5300, 6400, 7700, 9500, 12000, 15500,
                                         24000};

extern "C" int pacx_default_bands(int sample_rate, int n_mdct_lines, int32_t *band_lines, int32_t *n_bands)
{
    if (sample_rate <= 0 || n_mdct_lines <= 0 || !band_lines || !n_bands)
        return PACX_E_ARG;
    /* AssignMDCTLinesFromFreqLimits (coder/psychoac.py:106-124), same operations in the
       same order: every one is a correctly rounded IEEE operation or exact */
    const double width = (double)sample_rate / (double)(2 * n_mdct_lines);
    double centers[25], counts[25];
    for (int i = 0; i < 25; ++i)
        centers[i] = floor(kCbFreqLimits[i] / width - 0.5);
    for (int i = 0; i < 25; ++i)
        counts[i] = centers[i] - (i ? centers[i - 1] : -1.0);
    for (int i = 0; i < 25; ++i)
        if (kCbFreqLimits[i] > (double)sample_rate / 2.0) {
            double sum = 0.0;
            for (int k = 0; k < i; ++k)
                sum += counts[k];
            counts[i] = (double)n_mdct_lines - sum;
            for (int k = i + 1; k < 25; ++k)
                counts[k] = 0.0;
            break;
        }
    /* ScaleFactorBands (coder/psychoac.py:143-149): a band of <= 12 lines joins its right
       neighbour (the array is cast to int first, :141) */
    std::vector<long long> n(25);
    for (int i = 0; i < 25; ++i)
        n[i] = (long long)counts[i];
    size_t i = 1;
    while (i < n.size()) {
        if (n[i - 1] <= 12) {
            n[i] += n[i - 1];
            n.erase(n.begin() + (long)(i - 1));
        } else {
            ++i;
        }
    }
    for (size_t k = 0; k < n.size(); ++k)
        band_lines[k] = (int32_t)n[k];
    *n_bands = (int32_t)n.size();
    return PACX_OK;
}

extern "C" int pacx_abi_version(void) { return PACX_ABI_VERSION; }

extern "C" const char *pacx_last_error(const pacx_handle *h) { return h ? h->err.c_str() : g_create_err.c_str(); }

extern "C" int pacx_band_stride(const pacx_handle *h) { return h ? h->T.band_stride : PACX_E_ARG; }

extern "C" int pacx_payload_stride(const pacx_handle *h) { return h ? PACX_PAYLOAD_STRIDE : PACX_E_ARG; }

/* The bands need not reach the last MDCT line: above 48 kHz the critical-band table
 * ends at 24 kHz and the reference leaves the lines beyond it uncoded
 * (coder/psychoac.py:106-124).  Those lines map to the dummy band index nb, whose
 * allocation the kernels keep at zero. */
static int build_bands(pacx_handle *h, const int32_t *lines, int nb, int total,
                       const int32_t **d_lower, const int32_t **d_lines, const uint8_t **d_map, int *covered)
{
    std::vector<int32_t> lower(nb), cnt(lines, lines + nb);
    std::vector<uint8_t> map(total, (uint8_t)nb);
    int at = 0;
    for (int b = 0; b < nb; ++b) {
        lower[b] = at;
        if (cnt[b] <= 0)
            return fail(h, PACX_E_ARG, "band with no lines");
        for (int k = 0; k < cnt[b] && at + k < total; ++k)
            map[at + k] = (uint8_t)b;
        at += cnt[b];
    }
    if (at > total)
        return fail(h, PACX_E_ARG, "band line counts exceed the number of MDCT lines");
    if (at < total && nb >= PACX_MAX_BANDS)
        return fail(h, PACX_E_UNSUPPORTED, "at most 31 bands when the bands do not cover every line");
    *covered = at;
    int rc;
    if ((rc = upload(h, lower.data(), nb, d_lower))) return rc;
    if ((rc = upload(h, cnt.data(), nb, d_lines))) return rc;
    return upload(h, map.data(), total, d_map);
}

/* bytes of one record (coder/pacfile.py:342-361, 552-565): per (sub-)block the overall scale, a size and a scale
   factor per band and mant_bits of mantissas; eight of them in a short frame; plus 4 bits, rounded up */
static long long record_bytes(int n_scale_bits, int n_mant_size_bits, int nb, long long mant_bits, bool is_short)
{
    const long long unit = n_scale_bits + (long long)nb * (n_mant_size_bits + n_scale_bits) + mant_bits;
    return ((is_short ? PACX_SUB : 1) * unit + 4 + 7) >> 3;
}

extern "C" int pacx_create(const pacx_config *cfg, pacx_handle **out)
{
    if (!cfg || !out)
        return fail(nullptr, PACX_E_ARG, "pacx_create: null argument");
    *out = nullptr;
    if (cfg->abi_version != PACX_ABI_VERSION)
        return fail(nullptr, PACX_E_ARG, "pacx_create: abi_version mismatch");
    if (cfg->n_lines_long != PACX_M_LONG || cfg->n_lines_short != PACX_M_SHORT)
        return fail(nullptr, PACX_E_UNSUPPORTED,
                    "pacx_create: kernels are built for nMDCTLines 1024 (long) / 128 (short)");
    if (cfg->n_bands_long < 1 || cfg->n_bands_long > PACX_MAX_BANDS || cfg->n_bands_short < 1 ||
        cfg->n_bands_short > 8 || !cfg->band_lines_long || !cfg->band_lines_short)
        return fail(nullptr, PACX_E_ARG, "pacx_create: band tables missing or too large");
    if (cfg->n_scale_bits < 1 || cfg->n_scale_bits > 4 || cfg->n_mant_size_bits < 1 ||
        cfg->n_mant_size_bits > 16 || cfg->sample_rate <= 0)
        return fail(nullptr, PACX_E_UNSUPPORTED, "pacx_create: nScaleBits must be 1..4, nMantSizeBits 1..16");
    int n_dev = 0;
    if (hipGetDeviceCount(&n_dev) != hipSuccess || n_dev <= 0)
        return fail(nullptr, PACX_E_HIP, "pacx_create: no HIP device visible (this library has no CPU path)");
    if (cfg->device < 0 || cfg->device >= n_dev)
        return fail(nullptr, PACX_E_ARG, "pacx_create: device ordinal out of range");

    pacx_handle *h = new pacx_handle();      /* every field zero: no workspace, no streams, no events */
    h->device = cfg->device;
    h->force = read_overrides();
    h->tables_exact = 1;
    memset(&h->T, 0, sizeof(h->T));
    int rc = PACX_OK;
#define TRY(x) do { rc = (x); if (rc) { g_create_err = h->err; pacx_destroy(h); return rc; } } while (0)
    {
        hipError_t e = hipSetDevice(cfg->device);
        if (e != hipSuccess) {
            g_create_err = std::string("hipSetDevice: ") + hipGetErrorString(e);
            delete h;
            return PACX_E_HIP;
        }
    }
    if (hipStreamCreateWithFlags(&h->side_stream, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&h->ev_fork, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&h->ev_join, hipEventDisableTiming) != hipSuccess ||
        hipStreamCreateWithFlags(&h->short_stream, hipStreamNonBlocking) != hipSuccess ||
        hipStreamCreateWithFlags(&h->spare_stream, hipStreamNonBlocking) != hipSuccess ||
        hipEventCreateWithFlags(&h->ev_short_done, hipEventDisableTiming) != hipSuccess ||
        hipEventCreateWithFlags(&h->ev_lists, hipEventDisableTiming) != hipSuccess) {
        g_create_err = "pacx_create: could not create the side stream / events";
        pacx_destroy(h);
        return PACX_E_HIP;
    }
    {
        hipDeviceProp_t prop;
        h->n_cu = (hipGetDeviceProperties(&prop, cfg->device) == hipSuccess && prop.multiProcessorCount > 0)
                      ? prop.multiProcessorCount : 256;
    }
    PacxTables &T = h->T;
    const int NL = PACX_N_LONG, NS = PACX_N_SHORT, ML = PACX_M_LONG, MS = PACX_M_SHORT;
    const double sr = cfg->sample_rate;

    /* windows */
    std::vector<double> wl(4 * NL), ws(NS), hl(NL), hs(NS);
    if (cfg->win_long) {
        memcpy(wl.data(), cfg->win_long, sizeof(double) * 4 * NL);
    } else {
        /* coder/window.py:61-92: np.concatenate of sine halves, ones and zeros */
        const std::vector<double> sl = gen_table(PACX_GEN_SINE_LONG, NL), ss = gen_table(PACX_GEN_SINE_SHORT, NS);
        const int pad = NL / 4 - NS / 4;
        for (int i = 0; i < NL; ++i) {
            wl[i] = sl[i];
            double st;                                    /* start window, coder/window.py:67-69 */
            if (i < NL / 2) st = sl[i];
            else if (i < NL / 2 + pad) st = 1.0;
            else if (i < NL / 2 + pad + NS / 2) st = ss[NS / 2 + (i - NL / 2 - pad)];
            else st = 0.0;
            wl[NL + i] = st;
            double ssw;                                   /* start-stop, coder/window.py:88-90 */
            if (i < pad) ssw = 0.0;
            else if (i < pad + NS / 2) ssw = ss[i - pad];
            else if (i < pad + NS / 2 + 2 * pad) ssw = 1.0;
            else if (i < pad + NS + 2 * pad) ssw = ss[NS / 2 + (i - pad - NS / 2 - 2 * pad)];
            else ssw = 0.0;
            wl[3 * NL + i] = ssw;
        }
        for (int i = 0; i < NL; ++i)
            wl[2 * NL + i] = wl[NL + (NL - 1 - i)];       /* stop = flipped start */
    }
    if (cfg->win_short) memcpy(ws.data(), cfg->win_short, sizeof(double) * NS);
    else ws = gen_table(PACX_GEN_SINE_SHORT, NS);
    if (cfg->hann_long) memcpy(hl.data(), cfg->hann_long, sizeof(double) * NL);
    else hl = gen_table(PACX_GEN_HANN_LONG, NL);
    if (cfg->hann_short) memcpy(hs.data(), cfg->hann_short, sizeof(double) * NS);
    else hs = gen_table(PACX_GEN_HANN_SHORT, NS);
    {
        std::vector<double> kl = gen_table(PACX_GEN_KBD_LONG, NL), ks = gen_table(PACX_GEN_KBD_SHORT, NS);
        if (cfg->kbd_long) memcpy(kl.data(), cfg->kbd_long, sizeof(double) * NL);
        if (cfg->kbd_short) memcpy(ks.data(), cfg->kbd_short, sizeof(double) * NS);
        TRY(upload(h, kl.data(), kl.size(), &T.kbd_long));
        TRY(upload(h, ks.data(), ks.size(), &T.kbd_short));
    }
    TRY(upload(h, wl.data(), wl.size(), &T.win_long));
    TRY(upload(h, ws.data(), ws.size(), &T.win_short));
    TRY(upload(h, hl.data(), hl.size(), &T.hann_long));
    TRY(upload(h, hs.data(), hs.size(), &T.hann_short));
    {
        std::vector<double> ones(NL, 1.0);
        TRY(upload(h, ones.data(), ones.size(), &T.ones));
        /* Hann tables with the PCM scale folded in (see k_psy.hip) */
        std::vector<double> hlp(NL), hsp(NS);
        for (int i = 0; i < NL; ++i) hlp[i] = hl[i] * (2.0 / 65535.0);
        for (int i = 0; i < NS; ++i) hsp[i] = hs[i] * (2.0 / 65535.0);
        TRY(upload(h, hlp.data(), hlp.size(), &T.hann_long_pcm));
        TRY(upload(h, hsp.data(), hsp.size(), &T.hann_short_pcm));
    }

    /* twiddles */
    {
        std::vector<double2> t;
        t = unit_circle(512, 8, 1, 8192);  TRY(upload(h, t.data(), t.size(), &T.tw_long));
        t = unit_circle(64, 8, 1, 1024);   TRY(upload(h, t.data(), t.size(), &T.tw_short));
        t = unit_circle(512, 2, 0, 512);   TRY(upload(h, t.data(), t.size(), &T.w512));
        /* the two tables of the long side chain's real-FFT split are made exactly
           symmetric (a handful of entries move by one ulp), so that the kernel derives
           W1024^(512-k) = -conj(W1024^k) and W2048^(k+512) = -j W2048^k from the entry it
           has already loaded instead of fetching them */
        t = unit_circle(512, 2, 0, 1024);
        for (int k = 1; k < 256; ++k)
            t[512 - k] = make_double2(-t[k].x, t[k].y);
        t[256].x = 0.0;
        TRY(upload(h, t.data(), t.size(), &T.w1024));
        t = unit_circle(1025, 2, 0, 2048);
        for (int k = 0; k <= 512; ++k)
            t[k + 512] = make_double2(t[k].y, -t[k].x);
        TRY(upload(h, t.data(), t.size(), &T.w2048));
        t = unit_circle(64, 2, 0, 128);    TRY(upload(h, t.data(), t.size(), &T.w128));
        t = unit_circle(129, 2, 0, 256);   TRY(upload(h, t.data(), t.size(), &T.w256));
    }

    /* psychoacoustic tables at the MDCT line frequencies (coder/psychoac.py:183-184) */
    {
        std::vector<double> bl(ML), tl(ML), bs(MS), ts(MS);
        /* NULL tables: the built-in NumPy-evaluated copies where the sample rate has them,
           else the C math library (pacx_tables_exact() then says 0) */
        const int ri = gen_rate_index(cfg->sample_rate);
        const double *g_bl = ri >= 0 ? (const double *)PACX_GEN_BARK_LONG + (size_t)ri * ML : nullptr;
        const double *g_tl = ri >= 0 ? (const double *)PACX_GEN_THRESH_LONG + (size_t)ri * ML : nullptr;
        const double *g_bs = ri >= 0 ? (const double *)PACX_GEN_BARK_SHORT + (size_t)ri * MS : nullptr;
        const double *g_ts = ri >= 0 ? (const double *)PACX_GEN_THRESH_SHORT + (size_t)ri * MS : nullptr;
        if (ri < 0 && (!cfg->bark_long || !cfg->thresh_long || !cfg->bark_short || !cfg->thresh_short))
            h->tables_exact = 0;
        for (int k = 0; k < ML; ++k) {
            const double f = (sr / (2 * ML)) * (k + 0.5);
            bl[k] = cfg->bark_long ? cfg->bark_long[k] : (g_bl ? g_bl[k] : pacx_bark(f));
            tl[k] = cfg->thresh_long ? cfg->thresh_long[k] : (g_tl ? g_tl[k] : pacx_thresh_quiet(f));
        }
        for (int k = 0; k < MS; ++k) {
            const double f = (sr / (2 * MS)) * (k + 0.5);
            bs[k] = cfg->bark_short ? cfg->bark_short[k] : (g_bs ? g_bs[k] : pacx_bark(f));
            ts[k] = cfg->thresh_short ? cfg->thresh_short[k] : (g_ts ? g_ts[k] : pacx_thresh_quiet(f));
        }
        TRY(upload(h, bl.data(), bl.size(), &T.bark_long));
        TRY(upload(h, tl.data(), tl.size(), &T.thresh_long));
        TRY(upload(h, bs.data(), bs.size(), &T.bark_short));
        TRY(upload(h, ts.data(), ts.size(), &T.thresh_short));
    }
    /* FFT power normalisation 4/(N^2 mean(np.hanning(N)^2)) and rfftfreq step */
    auto hanning_norm = [](int n) {
        long double acc = 0;
        for (int i = 0; i < n; ++i) {
            const long double w = 0.5L - 0.5L * cosl(2.0L * 3.14159265358979323846264338327950288L * i / (n - 1));
            acc += w * w;
        }
        return (double)(4.0L / ((long double)n * n * (acc / n)));
    };
    (void)hanning_norm;       /* kept as the formula; the built-in values are NumPy's */
    T.norm_long = cfg->fft_norm_long != 0.0 ? cfg->fft_norm_long : ((const double *)PACX_GEN_FFT_NORM)[0];
    T.norm_short = cfg->fft_norm_short != 0.0 ? cfg->fft_norm_short : ((const double *)PACX_GEN_FFT_NORM)[1];
    T.fstep_long = cfg->fft_freq_step_long != 0.0 ? cfg->fft_freq_step_long : 1.0 / (NL * (1.0 / sr));
    T.fstep_short = cfg->fft_freq_step_short != 0.0 ? cfg->fft_freq_step_short : 1.0 / (NS * (1.0 / sr));

    {
        /* Bark of the long side-chain FFT's bin frequencies: a masker made of bins i-1 and i has its
           Bark value between entries i-1 and i (the kernel adds a margin) */
        std::vector<double> bb(NL / 2 + 1);
        for (int i = 0; i <= NL / 2; ++i)
            bb[i] = pacx_bark((double)i * T.fstep_long);
        TRY(upload(h, bb.data(), bb.size(), &T.bark_bin_long));
    }
    T.nb_long = cfg->n_bands_long;
    T.nb_short = cfg->n_bands_short;
    int covered_long = ML, covered_short = MS;
    TRY(build_bands(h, cfg->band_lines_long, T.nb_long, ML, &T.band_lower_long, &T.band_lines_long,
                    &T.line_band_long, &covered_long));
    TRY(build_bands(h, cfg->band_lines_short, T.nb_short, MS, &T.band_lower_short, &T.band_lines_short,
                    &T.line_band_short, &covered_short));
    if (covered_short < MS && T.nb_short >= 8) {
        g_create_err = "pacx_create: at most 7 short bands when they do not cover every line";
        pacx_destroy(h);
        return PACX_E_UNSUPPORTED;
    }
    T.band_stride = T.nb_long > PACX_SUB * T.nb_short ? T.nb_long : PACX_SUB * T.nb_short;
    T.n_scale_bits = cfg->n_scale_bits;
    T.n_mant_size_bits = cfg->n_mant_size_bits;
    T.target_bps = cfg->target_bits_per_sample;
    {
        /* the packers build a record in PACX_PAYLOAD_WORDS LDS words and copy it to a slot of PACX_PAYLOAD_STRIDE
           bytes: the longest record of these layouts and widths (every band at maxMantBits) has to fit */
        const int max_mant = T.n_mant_size_bits < 4 ? 1 << T.n_mant_size_bits : 16;
        const int ns = T.n_scale_bits, nm = T.n_mant_size_bits;
        const long long lon = record_bytes(ns, nm, T.nb_long, (long long)max_mant * covered_long, false);
        const long long sht = record_bytes(ns, nm, T.nb_short, (long long)max_mant * covered_short, true);
        const long long longest = lon > sht ? lon : sht;
        if (longest > PACX_PAYLOAD_STRIDE) {
            g_create_err = "pacx_create: the longest record of these band layouts at nScaleBits " + std::to_string(ns) +
                           ", nMantSizeBits " + std::to_string(nm) + " takes " + std::to_string(longest) +
                           " bytes, a payload slot holds " + std::to_string(PACX_PAYLOAD_STRIDE);
            pacx_destroy(h);
            return PACX_E_UNSUPPORTED;
        }
    }

    /* coding variant */
    T.guard = cfg->guard ? 1 : 0;
    T.use_vq = cfg->use_vq ? 1 : 0;
    T.use_sbr = cfg->use_sbr ? 1 : 0;
    T.first_omitted = T.nb_long;
    T.band_lines_long_alloc = T.band_lines_long;
    if (T.use_sbr) {
        /* sbr.omitted_bands (coder/sbr.py:6-9): bands starting at or above upperLine[-1] // 2 */
        std::vector<int32_t> alloc_lines(cfg->band_lines_long, cfg->band_lines_long + T.nb_long);
        const int cut = (covered_long - 1) / 2;      /* sfBands.upperLine[-1] // 2 */
        int at = 0;
        for (int b = 0; b < T.nb_long; ++b) {
            if (at >= cut) {
                if (T.first_omitted == T.nb_long)
                    T.first_omitted = b;
                alloc_lines[b] = 1;
            }
            at += cfg->band_lines_long[b];
        }
        if (T.nb_long - T.first_omitted > PACX_SUB) {
            g_create_err = "pacx_create: more than 8 SBR-omitted bands";
            pacx_destroy(h);
            return PACX_E_UNSUPPORTED;
        }
        TRY(upload(h, alloc_lines.data(), alloc_lines.size(), &T.band_lines_long_alloc));
    }
    PvqTables tab;                         /* device copies, for both views */
    memset(&tab, 0, sizeof(tab));
    tab.l_max = 1;
    const double *d_lt = nullptr;
    if (T.use_vq) {
        int l_max = 1;
        for (int b = 0; b < T.nb_long; ++b)
            l_max = cfg->band_lines_long[b] > l_max ? cfg->band_lines_long[b] : l_max;
        for (int b = 0; b < T.nb_short; ++b)
            l_max = cfg->band_lines_short[b] > l_max ? cfg->band_lines_short[b] : l_max;
        tab.l_max = l_max;
        PacxVqHostTables vt;
        /* NULL gain-shape tables: the built-in NumPy-evaluated copies (l_max <= 1024 always:
           a band cannot have more lines than the block) */
        pacx_vq_build(l_max, cfg->half_log2 ? cfg->half_log2 : (const double *)PACX_GEN_HALF_LOG2, &vt);
        if (vt.n_tab.empty()) {            /* l_max < 3: rows 0..2 are closed forms */
            vt.n_tab.push_back(0);
            vt.p_tab.push_back(0);
        }
        TRY(upload(h, vt.n_tab.data(), vt.n_tab.size(), &tab.n_tab));
        TRY(upload(h, vt.p_tab.data(), vt.p_tab.size(), &tab.p_tab));
        TRY(upload(h, vt.row_off.data(), vt.row_off.size(), &tab.row_off));
        TRY(upload(h, vt.k_of.data(), vt.k_of.size(), &tab.k_of));
        TRY(upload(h, vt.w_of.data(), vt.w_of.size(), &tab.w_of));
        TRY(upload(h, vt.half_log2.data(), vt.half_log2.size(), &tab.half_log2));
        h->vq_view.resize(pacx_vq_view_size());
        std::vector<int32_t> sizes_long(cfg->band_lines_long, cfg->band_lines_long + T.nb_long);
        for (int b = T.first_omitted; b < T.nb_long; ++b)
            sizes_long[b] = 1;
        /* log2(tan(theta_q) + eps) of the quantised split angles (bit_allocation_ms) */
        std::vector<double> lt((1u << PACX_VQ_THETA_TABLE_BITS) - 1, 0.0);
        memcpy(lt.data(), cfg->vq_log2_tan ? cfg->vq_log2_tan : (const double *)PACX_GEN_VQ_LOG2_TAN,
               sizeof(double) * lt.size());
        static_assert(sizeof(PACX_GEN_VQ_LOG2_TAN) / 8 == (1u << PACX_VQ_THETA_TABLE_BITS) - 1, "log2-tan table");
        TRY(upload(h, lt.data(), lt.size(), &d_lt));
        pacx_vq_view_fill(h->vq_view.data(), tab, cfg->log_mu1 != 0.0 ? cfg->log_mu1 : ((const double *)PACX_GEN_LOG_MU1)[0],
                          d_lt, sizes_long.data(), T.nb_long, cfg->band_lines_short, T.nb_short);
    }
    if (T.use_vq || T.use_sbr) {
        /* decode side: Gaussian weights of gaussian_filter1d(sigma=200) (radius
           int(4*200 + 0.5)) and the MDCT line frequencies of Decode_SBR (scalar-mantissa SBR
           handles: these two alone, for k_sbr_recon) */
        const int gr = cfg->sbr_gauss ? cfg->sbr_gauss_radius : 800;
        if (gr < 1 || gr > 4096) {
            g_create_err = "pacx_create: sbr_gauss_radius out of range";
            pacx_destroy(h);
            return PACX_E_ARG;
        }
        std::vector<double> gw(2 * gr + 1), lf(ML);
        static_assert(sizeof(PACX_GEN_SBR_GAUSS) / 8 == 2 * 800 + 1, "gaussian weights");
        memcpy(gw.data(), cfg->sbr_gauss ? cfg->sbr_gauss : (const double *)PACX_GEN_SBR_GAUSS,
               sizeof(double) * gw.size());
        for (int k = 0; k < ML; ++k)
            lf[k] = cfg->line_freq_long ? cfg->line_freq_long[k] : (k + 0.5) * (sr / (2 * ML));
        const double *d_gw, *d_lf;
        TRY(upload(h, gw.data(), gw.size(), &d_gw));
        TRY(upload(h, lf.data(), lf.size(), &d_lf));
        h->vqdec_view.resize(pacx_vqdec_view_size());
        pacx_vqdec_view_fill(h->vqdec_view.data(), tab, d_lt, d_gw, gr, d_lf, cfg->band_lines_long, T.nb_long,
                             cfg->band_lines_short, T.nb_short);
    }
#undef TRY
    *out = h;
    return PACX_OK;
}

static void drain_internal(pacx_handle *h)
{
    for (hipStream_t s2 : {h->side_stream, h->short_stream})
        if (s2)
            (void)hipStreamSynchronize(s2);
}

static int post_launch_forked(pacx_handle *h, const char *what)
{
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) {
        drain_internal(h);
        return fail(h, PACX_E_HIP, std::string(what) + ": " + hipGetErrorString(e));
    }
    return PACX_OK;
}

/* The handle's device buffers, in groups.  Each group has a capacity of its own (channel-frames; bytes for the index,
   states for the solve) and only ever grows, on the first call that needs more.  The main workspace is what every
   encode step uses (pacx_reserve); the others belong to the entry points that name them. */
enum { GROW_NONE = -1, GROW_MANT, GROW_VQ_UNITS, GROW_DEC_BLOCKS, GROW_DEC_LINES, GROW_NMR, GROW_INDEX, GROW_SOLVE,
       GROW_VQ_BAND, GROW_MAIN, GROW_N };
struct GrowGroup {
    long long *cap;
    const long long *follows;         /* once this capacity is above zero the group is kept as large as the main workspace
                                         (reserve); nullptr: it grows only where an entry point asks */
    /* n units of capacity take unit * (n / div + add) bytes (none: the buffer is not allocated); p == nullptr ends the group */
    struct { void **p; size_t unit, div = 1, add = 0; } buf[10];
};

/* pacx_vq_band_curve_batch's buffers of one pass, carved out of one allocation: n entries of every array, each
   entry a multiple of 16 bytes */
struct VqBandWs {
    uint8_t *payload;                 /* [n][PACX_PAYLOAD_STRIDE] what the coder wrote */
    double *noise, *mask, *nmr;       /* [n][band_stride] k_nmr's rows */
    int32_t *alloc, *dec_alloc;       /* [n][band_stride] the pass's allocation (in and out), the decoder's copy */
    int32_t *dec_overall, *budget;    /* [n][8] the overall scales the decoder read; the cap budgets */
    int32_t *n_bytes;                 /* [n] */
    uint32_t *status;                 /* [n] the pass's own status words */
    uint8_t *cf_flags;                /* [n] the flags the decoder read */
};

static size_t vq_band_ws(const PacxTables &T, char *base, long long n, VqBandWs *ws)
{
    const size_t rows = ((size_t)T.band_stride * sizeof(double) + 15) & ~(size_t)15;
    const size_t ints = ((size_t)T.band_stride * sizeof(int32_t) + 15) & ~(size_t)15;
    const size_t unit[] = {PACX_PAYLOAD_STRIDE, rows, rows, rows, ints, ints, PACX_SUB * sizeof(int32_t),
                           PACX_SUB * sizeof(int32_t), 16, 16, 16};
    static_assert(PACX_PAYLOAD_STRIDE % 16 == 0, "every array of the carve starts 16-byte aligned");
    char *at[sizeof(unit) / sizeof(unit[0])];
    size_t total = 0;
    for (size_t i = 0; i < sizeof(unit) / sizeof(unit[0]); ++i) {
        at[i] = base + (size_t)n * total;
        total += unit[i];
    }
    if (ws)
        *ws = {(uint8_t *)at[0], (double *)at[1], (double *)at[2], (double *)at[3], (int32_t *)at[4], (int32_t *)at[5],
               (int32_t *)at[6], (int32_t *)at[7], (int32_t *)at[8], (uint32_t *)at[9], (uint8_t *)at[10]};
    return total;                                  /* bytes per channel-frame */
}

static GrowGroup grow_group(pacx_handle *h, int which)
{
    switch (which) {
    case GROW_MAIN:
        return {&h->ws_cf, nullptr,
                {{(void **)&h->ws_lines, PACX_M_LONG * sizeof(double)},
                 {(void **)&h->ws_smr, h->T.band_stride * sizeof(double)},
                 {(void **)&h->ws_peaks, PACX_MAX_PEAKS * sizeof(PacxPeak)},
                 {(void **)&h->ws_npeaks, PACX_SUB * sizeof(int32_t)},
                 {(void **)&h->ws_nkept, PACX_SUB * sizeof(int32_t)},
                 {(void **)&h->ws_overall, PACX_SUB * sizeof(int32_t)},
                 {(void **)&h->ws_chunks, sizeof(long long), 256, 2},                   /* [ws_cf/256 + 2] */
                 {(void **)&h->ws_offs, sizeof(long long), 1, 1},                       /* [ws_cf + 1] */
                 {(void **)&h->ws_lists, 2 * sizeof(int32_t), 1, 1},                    /* [2*ws_cf + 2] */
                 {(void **)&h->ws_sbr_mean, h->T.use_sbr ? PACX_SUB * sizeof(double) : 0}}};
    /* a handle that has served pacx_vq_band_curve_batch keeps its pass buffers and the decoder's lines as large as the
       workspace */
    case GROW_VQ_BAND:
        return {&h->ws_vqb_cf, &h->ws_vqb_cf, {{(void **)&h->ws_vqb, vq_band_ws(h->T, nullptr, 0, nullptr)}}};
    case GROW_MANT:
        return {&h->ws_mant_cf, nullptr, {{(void **)&h->ws_mant, PACX_M_LONG * sizeof(int32_t)}}};
    case GROW_VQ_UNITS:
        return {&h->ws_vq_cf, nullptr,
                {{(void **)&h->ws_unit_words, PACX_SUB * PACX_PAYLOAD_WORDS * sizeof(unsigned)},
                 {(void **)&h->ws_unit_bits, PACX_SUB * 2 * sizeof(int32_t)}}};
    /* the decoders' own workspaces: windowed blocks when the caller wants PCM only; lines + SBR flags (+ status words) */
    case GROW_DEC_BLOCKS:
        return {&h->ws_blocks_cf, nullptr, {{(void **)&h->ws_blocks, PACX_N_LONG * sizeof(double)}}};
    case GROW_DEC_LINES:
        return {&h->ws_dec_cf, &h->ws_vqb_cf,
                {{(void **)&h->ws_dec_lines, PACX_M_LONG * sizeof(double)},
                 {(void **)&h->ws_dec_sbr, 1},
                 {(void **)&h->ws_dec_status, sizeof(uint32_t)}}};
    /* pacx_nmr_batch: the masked threshold of every line; pacx_rate_curve_batch: its status words as well.  A handle
       that has served either keeps them as large as the workspace */
    case GROW_NMR:
        return {&h->ws_thr_cf, &h->ws_thr_cf,
                {{(void **)&h->ws_thr, PACX_M_LONG * sizeof(double)}, {(void **)&h->ws_rate_status, sizeof(uint32_t)}}};
    case GROW_SOLVE:
        return {&h->ws_solve_n, nullptr,
                {{(void **)&h->ws_solve, pacx_rate_solve_ws_bytes()},
                 {(void **)&h->ws_seg, 3 * sizeof(long long)},
                 {(void **)&h->ws_bucket, pacx_bucket_ws_bytes(), (size_t)1 << 62, 1},               /* [1] */
                 {(void **)&h->ws_pin, pacx_pin_ws_unit(), 1, pacx_pin_ws_head() / pacx_pin_ws_unit()}}};
    default:
        return {&h->ws_index_bytes, nullptr, {{(void **)&h->ws_index, 1}}};
    }
}

static void free_group(const GrowGroup &g)
{
    for (const auto &b : g.buf)
        if (b.p && *b.p) {
            (void)hipFree(*b.p);
            *b.p = nullptr;
        }
    *g.cap = 0;
}

/* room for n units in one group, all or nothing: a failing hipMalloc (the main workspace of a 262 144-frame batch is
   8 GB) leaves the group with NO buffer and capacity 0 -- nothing leaks, and a later, smaller call allocates again */
static int grow(pacx_handle *h, int which, long long n)
{
    const GrowGroup g = grow_group(h, which);
    if (n <= *g.cap)
        return PACX_OK;
    HIP_TRY(h, hipDeviceSynchronize());
    free_group(g);
    for (const auto &b : g.buf) {
        const size_t bytes = b.p ? b.unit * ((size_t)n / b.div + b.add) : 0;
        if (!bytes)
            continue;
        hipError_t e = hipMalloc(b.p, bytes);
        if (e != hipSuccess) {
            *b.p = nullptr;
            free_group(g);
            (void)hipGetLastError();             /* the failed allocation must not poison the next launch check */
            return fail(h, PACX_E_HIP, std::string("pacx_reserve: hipMalloc of ") + std::to_string(bytes) +
                                           " bytes: " + hipGetErrorString(e) + " (workspace released)");
        }
    }
    *g.cap = n;
    return PACX_OK;
}

extern "C" void pacx_destroy(pacx_handle *h)
{
    if (!h)
        return;
    (void)hipSetDevice(h->device);
    for (hipStream_t s2 : {h->side_stream, h->short_stream, h->spare_stream})
        if (s2) {
            (void)hipStreamSynchronize(s2);
            (void)hipStreamDestroy(s2);
        }
    for (hipEvent_t e2 : {h->ev_short_done, h->ev_lists})
        if (e2)
            (void)hipEventDestroy(e2);
    if (h->ev_fork)
        (void)hipEventDestroy(h->ev_fork);
    if (h->ev_join)
        (void)hipEventDestroy(h->ev_join);
    for (int which = 0; which < GROW_N; ++which)
        free_group(grow_group(h, which));
    if (h->ev_seg) {
        (void)hipEventSynchronize(h->ev_seg);
        (void)hipEventDestroy(h->ev_seg);
    }
    if (h->seg_host)
        (void)hipHostFree(h->seg_host);
    for (void *p : h->owned)
        (void)hipFree(p);
    delete h;
}

/* the main workspace for n_cf channel-frames, and the groups that follow it; the device is the handle's already */
static int reserve(pacx_handle *h, long long n_cf)
{
    for (int which = 0; which < GROW_N; ++which) {
        const long long *follows = grow_group(h, which).follows;
        int rc;
        if (follows && *follows > 0 && (rc = grow(h, which, n_cf)))
            return rc;
    }
    return grow(h, GROW_MAIN, n_cf);
}

extern "C" int pacx_reserve(pacx_handle *h, int64_t n_cf)
{
    if (!h || n_cf < 0)
        return fail(h, PACX_E_ARG, "pacx_reserve: bad argument");
    if (n_cf > 0x7fffffffLL / PACX_SUB)
        return fail(h, PACX_E_ARG, "pacx_reserve: too many channel-frames for one call");
    HIP_TRY(h, hipSetDevice(h->device));
    return reserve(h, n_cf);
}

/* validate a pcm view; fills the device-side view and the fast-path flag */
static int check_pcm(pacx_handle *h, const pacx_pcm *in, PacxPcmView *v, int *fast, long long *n_cf)
{
    if (!in || (!in->data && in->n_frames != 0))
        return fail(h, PACX_E_ARG, "pcm view or data pointer is null");
    if (in->dtype != PACX_PCM_I16 && in->dtype != PACX_PCM_F64)
        return fail(h, PACX_E_ARG, "pcm dtype must be PACX_PCM_I16 or PACX_PCM_F64");
    if (in->n_channels < 1 || in->n_frames < 0 || in->sample_stride < 1 || in->frame_stride < 0 ||
        in->channel_stride < 0)
        return fail(h, PACX_E_ARG, "pcm view: bad channel count, frame count or stride");
    if (in->n_frames * in->n_channels > 0x7fffffffLL / PACX_SUB)
        return fail(h, PACX_E_ARG, "pcm view: too many channel-frames for one call");
    v->base = in->data;
    v->frame_stride = in->frame_stride;
    v->ch_stride = in->channel_stride;
    v->samp_stride = in->sample_stride;
    v->n_ch = in->n_channels;
    *fast = (in->dtype == PACX_PCM_I16 && in->sample_stride == 1 && ((uintptr_t)in->data % 16) == 0 &&
             in->frame_stride % 8 == 0 && in->channel_stride % 8 == 0);
    *n_cf = in->n_frames * in->n_channels;
    return PACX_OK;
}

static int post_launch(pacx_handle *h, const char *what)
{
    hipError_t e = hipGetLastError();
    if (e != hipSuccess)
        return fail(h, PACX_E_HIP, std::string(what) + ": " + hipGetErrorString(e));
    return PACX_OK;
}

/* ---- what the entry points refuse, stated once each; PACX_OK: not refused ---- */
static int scalar_only(pacx_handle *h, const char *what)
{
    if (h->T.use_vq || h->T.use_sbr)
        return fail(h, PACX_E_UNSUPPORTED, std::string(what) + ": scalar handles only (created without use_vq, use_sbr)");
    return PACX_OK;
}

static int vq_plain_only(pacx_handle *h, const char *what)
{
    if (!h->T.use_vq || h->T.use_sbr)
        return fail(h, PACX_E_UNSUPPORTED, std::string(what) + ": gain-shape handles without SBR only (created with use_vq, without use_sbr)");
    return PACX_OK;
}

/* instead: what a gain-shape handle's caller is pointed to */
static int not_vq(pacx_handle *h, const char *what, const char *instead)
{
    if (h->T.use_vq)
        return fail(h, PACX_E_UNSUPPORTED, std::string(what) + ": handle was created with use_vq (" + instead + ")");
    return PACX_OK;
}

static int vq_only(pacx_handle *h, const char *what)
{
    if (!h->T.use_vq)
        return fail(h, PACX_E_UNSUPPORTED, std::string(what) + ": handle was created without use_vq");
    return PACX_OK;
}

static bool cap_rate_ok(double max_bits_per_sample) { return max_bits_per_sample > 0.0 && max_bits_per_sample <= 16.0; }

static int check_cap_rate(pacx_handle *h, const char *what, double max_bits_per_sample)
{
    if (!cap_rate_ok(max_bits_per_sample))
        return fail(h, PACX_E_ARG, std::string(what) + ": max_bits_per_sample must lie in (0, 16]");
    return PACX_OK;
}

/* what one run of the gain-shape coder reads and writes beside the step's lines and overall scales: the allocation (in
   and out), status words, payload slots and record lengths; the omitted bands' means (SBR handles) and the entry log,
   or nullptr */
struct VqCode {
    int32_t *bit_alloc;
    uint32_t *status;
    uint8_t *payload;
    int32_t *n_bytes;
    const double *sbr_mean;
    pacx_vq_entry *log;
    int32_t *log_count;
    int log_cap;
};

/* What a call that takes a pacx_pcm knows about its batch, and what it hands to every launch of an encode's front end
   (frame lists -> long / short MDCT -> side chain -> mask): the launches below name only what differs between them --
   the stream, the part of a block-switched batch (0, PACX_PART_LONG, PACX_PART_SHORT), the fused tail.  An entry point
   strings the pieces together in its own order, view() .. reserve() .. init_outputs(), between its own checks: the
   order in which the checks answer is part of the interface (include/pacx.h, tests/test_gpu_api_refusals.py).  The
   schedules themselves (which stream, which order, which events) stay with the entry points: they differ for
   measured reasons. */
struct EncodeStep {
    pacx_handle *h;
    const uint8_t *frame_flags;
    int mixed;                        /* per-frame flags (without them every frame is a long sine block) */
    hipStream_t stream;               /* the caller's */
    /* view() */
    PacxPcmView v;
    int dtype, fast;
    long long n_frames, n_cf;
    int n_ch;
    /* reserve() */
    int32_t *list_long, *list_short, *counts;       /* h->ws_lists: long cf list, short cf list, the two counts */
    /* init_outputs() */
    int32_t *overall_scale;
    uint32_t *status;

    EncodeStep(pacx_handle *h_, const uint8_t *flags, void *stream_)
        : h(h_), frame_flags(flags), mixed(flags ? 1 : 0), stream((hipStream_t)stream_), n_cf(0), overall_scale(nullptr),
          status(nullptr)
    {
    }

    int view(const pacx_pcm *in)
    {
        const int rc = check_pcm(h, in, &v, &fast, &n_cf);
        if (rc)
            return rc;
        dtype = in->dtype;
        n_frames = in->n_frames;
        n_ch = in->n_channels;
        return PACX_OK;
    }

    /* the handle's device, its workspace for this batch and the groups the call names (GROW_NONE: none) */
    int reserve(std::initializer_list<int> groups = {})
    {
        HIP_TRY(h, hipSetDevice(h->device));
        int rc = ::reserve(h, n_cf);
        for (int which : groups)
            if (!rc && which != GROW_NONE)
                rc = grow(h, which, n_cf);
        if (rc)
            return rc;
        list_long = h->ws_lists;
        list_short = h->ws_lists + n_cf;
        counts = h->ws_lists + 2 * n_cf;
        return PACX_OK;
    }

    /* where the front end leaves its overall scales and status words, zeroed for the generic path */
    int init_outputs(int32_t *overall, uint32_t *status_)
    {
        overall_scale = overall;
        status = status_;
        if (!fast) {                               /* fast path: k_mdct_long_v2 initialises both itself */
            HIP_TRY(h, hipMemsetAsync(status, 0, (size_t)n_cf * sizeof(uint32_t), stream));
            HIP_TRY(h, hipMemsetAsync(overall_scale, 0, (size_t)n_cf * PACX_SUB * sizeof(int32_t), stream));
        }
        return PACX_OK;
    }

    void lists(hipStream_t st) const
    {
        pacx_launch_frame_lists(frame_flags, n_frames, n_ch, list_long, list_short, counts, st);
    }
    /* fast batches.  Long frames: persistent roofline kernel (k_mdct_long_v2; it also initialises status and the
       overall scales); short (CUR) frames: k_mdct_short */
    void mdct_long(hipStream_t st) const
    {
        pacx_launch_mdct_v2(h->T, v, frame_flags, n_cf, mixed, h->ws_lines, overall_scale, PACX_SUB, status, h->n_cu,
                            mixed ? list_long : nullptr, mixed ? counts : nullptr, st);
    }
    void mdct_short(hipStream_t st) const
    {
        pacx_launch_mdct(h->T, v, dtype, fast, frame_flags, n_cf, 0, 4, 0, h->ws_lines, overall_scale, PACX_SUB, status,
                         st);
    }
    /* every frame's MDCT on one stream */
    void mdct(hipStream_t st) const
    {
        if (fast) {
            mdct_long(st);
            if (mixed)
                mdct_short(st);
        } else {
            pacx_launch_mdct(h->T, v, dtype, fast, frame_flags, n_cf, 0, mixed, 0, h->ws_lines, overall_scale, PACX_SUB,
                             status, st);
        }
    }
    /* sbr: the side chain also leaves the omitted bands' means and folds max|FFT| into the overall scale the MDCT
       wrote (so it runs behind the MDCT on that MDCT's stream) */
    void side(int part, bool sbr, hipStream_t st) const
    {
        pacx_launch_side(h->T, v, dtype, fast, frame_flags, n_cf, 0, mixed | part, h->ws_peaks, h->ws_npeaks, h->ws_nkept,
                         sbr ? h->ws_sbr_mean : nullptr, sbr ? overall_scale : nullptr, st);
    }
    /* all-long fast batches without SBR: transform and side chain of a frame in one wave (k_front_long), which
       also initialises status and the overall scales */
    void front_long(hipStream_t st) const
    {
        pacx_launch_front_long(h->T, v, n_cf, h->ws_lines, overall_scale, status, h->ws_peaks, h->ws_npeaks,
                               h->ws_nkept, st);
    }
    /* lines, SMRs and, with thr, the masked threshold of every line, all on one stream: frame lists, MDCT, side
       chain, mask */
    void front(double *thr, hipStream_t st) const
    {
        if (mixed)
            lists(st);
        mdct(st);
        side(0, false, st);
        pacx_launch_mask(h->T, frame_flags, n_ch, n_cf, 0, mixed, h->ws_peaks, h->ws_nkept, h->ws_lines, h->ws_smr, thr,
                         h->n_cu, list_long, list_short, counts, nullptr, st);
    }
    /* tail: the outputs of the work fused into the long mask kernel, or nullptr */
    void mask(int part, const MaskTail *tail, hipStream_t st) const
    {
        pacx_launch_mask(h->T, frame_flags, n_ch, n_cf, 0, mixed | part, h->ws_peaks, h->ws_nkept, h->ws_lines, h->ws_smr,
                         nullptr, h->n_cu, list_long, list_short, counts, tail, st);
    }
    /* the gain-shape coder on this batch's lines and overall scales; stage 1: k_vq_frame over the frames of a list, 2:
       what follows it, 0: both over every frame */
    void vq(const VqCode &c, int stage, const int32_t *cf_list, const int32_t *cf_count, hipStream_t st) const
    {
        pacx_launch_vq(h->T, h->vq_view.data(), frame_flags, n_ch, n_cf, h->ws_lines, overall_scale, c.bit_alloc, c.sbr_mean,
                       c.status, c.payload, PACX_PAYLOAD_STRIDE, c.n_bytes, h->ws_unit_words, h->ws_unit_bits, c.log,
                       c.log_count, c.log_cap, stage, cf_list, cf_count, h->force.vq_frame, h->force.vq_bfs, st);
    }
};

extern "C" int pacx_mdct_batch(pacx_handle *h, const pacx_pcm *in, const uint8_t *frame_flags,
                               int mode, double *lines, int32_t *max_scale, void *stream)
{
    if (!h)
        return PACX_E_ARG;
    EncodeStep s(h, frame_flags, stream);
    const int rc = s.view(in);
    if (rc || s.n_cf == 0)
        return rc;
    if (!lines)
        return fail(h, PACX_E_ARG, "pacx_mdct_batch: lines is null");
    if ((mode & PACX_MDCT_KBD) && (frame_flags || (mode & PACX_MDCT_PREWINDOWED)))
        return fail(h, PACX_E_ARG, "pacx_mdct_batch: PACX_MDCT_KBD takes no frame flags and no PREWINDOWED");
    HIP_TRY(h, hipSetDevice(h->device));
    const int short_blocks = (mode & PACX_MDCT_SHORT) ? 1 : 0;
    if (mode & PACX_MDCT_KBD) {              /* window override 2 = the KBD tables */
        pacx_launch_mdct(h->T, s.v, s.dtype, s.fast, nullptr, s.n_cf, short_blocks, 0, 2, lines, max_scale,
                         short_blocks ? PACX_SUB : 1, nullptr, s.stream);
        return post_launch(h, "pacx_mdct_batch");
    }
    if (s.fast && !short_blocks && !(mode & PACX_MDCT_PREWINDOWED)) {
        pacx_launch_mdct_v2(h->T, s.v, frame_flags, s.n_cf, 0, lines, max_scale, 1, nullptr, h->n_cu, nullptr, nullptr,
                            s.stream);
        return post_launch(h, "pacx_mdct_batch");     /* v2 handles all four long windows */
    }
    pacx_launch_mdct(h->T, s.v, s.dtype, s.fast, frame_flags, s.n_cf, short_blocks, 0,
                     (mode & PACX_MDCT_PREWINDOWED) ? 1 : 0, lines, max_scale,
                     short_blocks ? PACX_SUB : 1, nullptr, s.stream);
    return post_launch(h, "pacx_mdct_batch");
}

extern "C" int pacx_smr_batch(pacx_handle *h, const pacx_pcm *in, const double *lines, int short_blocks,
                              double *smr, double *threshold, int32_t *n_peaks, void *stream)
{
    if (!h)
        return PACX_E_ARG;
    EncodeStep s(h, nullptr, stream);
    int rc = s.view(in);
    if (rc || s.n_cf == 0)
        return rc;
    if (!lines || !smr)
        return fail(h, PACX_E_ARG, "pacx_smr_batch: lines or smr is null");
    if ((rc = s.reserve()))
        return rc;
    hipStream_t st = s.stream;
    const long long n_cf = s.n_cf;
    const int sb = short_blocks ? 1 : 0;
    pacx_launch_side(h->T, s.v, s.dtype, s.fast, nullptr, n_cf, sb, 0, h->ws_peaks, h->ws_npeaks, h->ws_nkept,
                     nullptr, nullptr, st);
    pacx_launch_mask(h->T, nullptr, s.n_ch, n_cf, sb, 0, h->ws_peaks, h->ws_nkept, lines, smr,
                     threshold, h->n_cu, nullptr, nullptr, nullptr, nullptr, st);
    if (n_peaks) {
        if (sb)
            HIP_TRY(h, hipMemcpyAsync(n_peaks, h->ws_npeaks, (size_t)n_cf * PACX_SUB * sizeof(int32_t),
                                      hipMemcpyDeviceToDevice, st));
        else
            HIP_TRY(h, hipMemcpy2DAsync(n_peaks, sizeof(int32_t), h->ws_npeaks, PACX_SUB * sizeof(int32_t),
                                        sizeof(int32_t), (size_t)n_cf, hipMemcpyDeviceToDevice, st));
    }
    return post_launch(h, "pacx_smr_batch");
}

extern "C" int pacx_smr_generic_batch(pacx_handle *h, int64_t n_blocks, int n_samples, const double *data,
                                      const double *lines, const pacx_smr_tables *t, double *smr, double *threshold,
                                      int32_t *n_peaks, void *stream)
{
    if (!h)
        return PACX_E_ARG;
    if (n_blocks == 0)
        return PACX_OK;
    if (n_blocks < 0 || !data || !lines || !smr || !t || !t->hann || !t->tw_cos || !t->tw_sin || !t->bark ||
        !t->quiet || !t->band_lower || !t->band_lines)
        return fail(h, PACX_E_ARG, "pacx_smr_generic_batch: bad argument");
    if (n_samples < 16 || n_samples > 8192 || (n_samples & 1) || t->n_bands < 1 || t->n_bands > PACX_MAX_BANDS)
        return fail(h, PACX_E_UNSUPPORTED, "pacx_smr_generic_batch: blocks of 16..8192 samples (even), 1..32 bands");
    if (pacx_smr_generic_lds(n_samples) > 150 * 1024)
        return fail(h, PACX_E_UNSUPPORTED, "pacx_smr_generic_batch: block too long for the LDS of a CU");
    HIP_TRY(h, hipSetDevice(h->device));
    pacx_launch_smr_generic(n_blocks, n_samples, t->n_bands, data, lines, t->hann, t->tw_cos, t->tw_sin, t->fft_norm,
                            t->fft_freq_step, t->bark, t->quiet, t->band_lower, t->band_lines, smr, threshold, n_peaks,
                            (hipStream_t)stream);
    return post_launch(h, "pacx_smr_generic_batch");
}

extern "C" int pacx_bitalloc_batch(pacx_handle *h, int64_t n_cf, int n_channels, const uint8_t *frame_flags,
                                   int short_blocks, const double *smr, int32_t *bit_alloc,
                                   uint32_t *status, void *stream)
{
    if (!h)
        return PACX_E_ARG;
    if (n_cf == 0)
        return PACX_OK;
    if (n_cf < 0 || n_channels < 1 || !smr || !bit_alloc)
        return fail(h, PACX_E_ARG, "pacx_bitalloc_batch: bad argument");
    HIP_TRY(h, hipSetDevice(h->device));
    pacx_launch_bitalloc(h->T, frame_flags, n_channels, n_cf, short_blocks ? 1 : 0, 0, 0, smr, bit_alloc, status,
                         (hipStream_t)stream);
    return post_launch(h, "pacx_bitalloc_batch");
}

extern "C" int pacx_quantize_batch(pacx_handle *h, int64_t n_cf, const double *lines,
                                   const int32_t *overall_scale, const int32_t *bit_alloc, int short_blocks,
                                   int32_t *scale_factor, int32_t *mantissa, void *stream)
{
    if (!h)
        return PACX_E_ARG;
    if (n_cf == 0)
        return PACX_OK;
    if (n_cf < 0 || !lines || !overall_scale || !bit_alloc || !scale_factor || !mantissa)
        return fail(h, PACX_E_ARG, "pacx_quantize_batch: bad argument");
    HIP_TRY(h, hipSetDevice(h->device));
    pacx_launch_quantize(h->T, nullptr, 1, n_cf, short_blocks ? 1 : 0, 0, lines, overall_scale,
                         short_blocks ? PACX_SUB : 1, bit_alloc, scale_factor, mantissa, (hipStream_t)stream);
    return post_launch(h, "pacx_quantize_batch");
}

static int encode_scalar(pacx_handle *h, const pacx_pcm *in, const uint8_t *frame_flags,
                         int32_t *overall_scale, int32_t *scale_factor, int32_t *bit_alloc,
                         int32_t *mantissa, uint32_t *status, uint8_t *payload, int32_t *n_bytes,
                         void *stream, const char *what)
{
    if (!h)
        return PACX_E_ARG;
    EncodeStep s(h, frame_flags, stream);
    int rc = s.view(in);
    if (rc || s.n_cf == 0)
        return rc;
    if (!overall_scale || !scale_factor || !bit_alloc || !status || (!payload && !mantissa) ||
        (payload && !n_bytes))
        return fail(h, PACX_E_ARG, std::string(what) + ": null output pointer");
    if ((rc = not_vq(h, what, "call pacx_encode_vq_batch")))
        return rc;
    const PacxTables &T = h->T;
    const long long n_cf = s.n_cf;
    const int fast = s.fast, mixed = s.mixed;
    hipStream_t st = s.stream;
    /* k_tail_short (and the tails of the long frames) pack from registers; only the separate-kernel fallback for
       layouts with more than 8 short bands (k_quantize<128> -> k_pack) reads the mantissas back from memory.  Round 3:
       the workspace copy is no longer written when nobody asked for mantissas (it was 4 KB per channel-frame of HBM
       writes in every block-switched step) */
    const bool own_mant = !mantissa && mixed && T.nb_short > 8;
    if ((rc = s.reserve({own_mant ? GROW_MANT : GROW_NONE})))
        return rc;
    if (own_mant)
        mantissa = h->ws_mant;
    if ((rc = s.init_outputs(overall_scale, status)))
        return rc;
    /* mixed streams: compacted lists of the long- and of the short-coded frames -- every
       persistent kernel below walks its own list.  The two-stream schedule forks first: the side
       chains and the short-block MDCT go by the flags alone and start while the lists are made */
    const bool split = mixed && fast && !h->T.use_sbr && h->force.split_short != 0;
    if (split)
        HIP_TRY(h, hipEventRecord(h->ev_fork, st));
    if (mixed)
        s.lists(st);
    if (split)
        HIP_TRY(h, hipEventRecord(h->ev_lists, st));
    /* long frames: masked threshold, SMRs, BitAlloc, scale factors / mantissas and the payload
       in ONE kernel (k_mask<1024, true>: the wave that has a frame's SMRs goes on with it; the
       lines are read from HBM once and the SMRs never leave the chip: 210 MB of HBM traffic per
       8192-frame step instead of 280), or the tail in k_tail_long behind a kernel boundary.
       Measured A/B on the same box: block-switched batches are 2 % faster
       fused; all-long batches 2 % faster UNFUSED (the separate tail kernel pairs two frames per
       wave for BitAlloc and runs at 20 waves per CU instead of 12) -- the default follows the
       clock, PACX_FUSE_TAIL=1 / 0 forces either. */
    const int fuse = h->force.fuse_tail >= 0 ? h->force.fuse_tail : mixed;
    MaskTail mt;
    mt.overall = overall_scale; mt.bit_alloc = bit_alloc; mt.scale_factor = scale_factor; mt.mantissa = mantissa;
    mt.status = status; mt.payload = payload; mt.n_bytes = n_bytes; mt.payload_stride = PACX_PAYLOAD_STRIDE;
    /* the tail as kernels of its own: the frames of a list (the short-coded ones), or every frame that skip_long
       leaves */
    auto tail = [&](const int32_t *cf_list, const int32_t *cf_count, int skip_long, hipStream_t s2) {
        pacx_launch_tail(T, frame_flags, s.n_ch, n_cf, h->ws_smr, h->ws_lines, overall_scale, bit_alloc, scale_factor,
                         mantissa, status, payload, PACX_PAYLOAD_STRIDE, n_bytes, cf_list, cf_count, skip_long, s2);
    };
    if (T.use_sbr) {
        /* scalar mantissas in an SBR file (coder/codec.py:426-482, 529-555; long blocks only, short
           ones take the plain path, coder/pacfile.py:639-643): the side chain folds max|FFT| into
           the overall scale the MDCT wrote, so it runs behind the MDCT on one stream; BitAlloc counts
           the omitted bands as one line and budgets from the full block (T.use_sbr in the tail
           kernels), and a frame whose omitted band gets bits is where the reference raises:
           PACX_ST_REF_RAISES, n_bytes 0.  Not a tuned path -- the reference's driver never selects it. */
        s.mdct(st);
        s.side(0, true, st);
        s.mask(0, nullptr, st);
        tail(s.list_short, s.counts + 1, 0, st);
        return post_launch(h, what);
    }
    if (split) {
        /* A block-switched batch is two independent chains that touch disjoint frames:
             long-coded :  k_side_long,  k_mdct_long_v2 ->  k_mask<1024> (+ tail)     on the caller's stream
             short-coded:  k_side_short, k_mdct_short   ->  k_mask<128> -> k_tail_short on short_stream
           Every one of these kernels is latency-bound at the occupancy its registers and LDS allow and none fills
           the chip with half of the frames, so the two chains run side by side and meet again before the body
           gather.  Each side chain runs on its chain's own stream: with four streams per handle (a side stream
           per chain) the short side chain of one handle landed on the other's short-chain hardware queue with two
           steps in flight (kernel trace), and alone the forks and joins cost more than the overlap
           of a side chain with its 40 us transform: bs128 33.9 -> 35.4 M cf/s with two steps in flight, 25.9 ->
           30.7 M with one. */
        HIP_TRY_FORKED(h, hipStreamWaitEvent(h->short_stream, h->ev_fork, 0));
        s.side(PACX_PART_LONG, false, st);
        s.side(PACX_PART_SHORT, false, h->short_stream);
        /* short chain */
        s.mdct_short(h->short_stream);
        HIP_TRY_FORKED(h, hipStreamWaitEvent(h->short_stream, h->ev_lists, 0));
        s.mask(PACX_PART_SHORT, nullptr, h->short_stream);
        tail(s.list_short, s.counts + 1, 1, h->short_stream);
        HIP_TRY_FORKED(h, hipEventRecord(h->ev_short_done, h->short_stream));
        /* long chain */
        s.mdct_long(st);
        s.mask(PACX_PART_LONG, fuse ? &mt : nullptr, st);
        if (!fuse)
            tail(nullptr, nullptr, 2, st);      /* every long-coded frame */
        HIP_TRY_FORKED(h, hipStreamWaitEvent(st, h->ev_short_done, 0));       /* both chains done */
        return post_launch_forked(h, what);
    }
    /* Fast all-long batches: MDCT and side chain in ONE kernel (k_front_long), the step a plain chain on the
       caller's stream whatever fork_side says.  HIP puts a handle's two streams on one hardware queue, so the
       forked step was a serial chain already -- side chain, then the transform, which holds a whole CU's LDS and
       leaves the vector unit three-quarters idle; in the side chain's wave the transform's memory traffic runs
       under arithmetic.  Same bits (tests/test_gpu_fused_front.py); measured in DESIGN.md 5.4; PACX_FUSE_FRONT=0 / 1
       forces either. */
    if (!mixed && fast && (h->force.fuse_front >= 0 ? h->force.fuse_front : PACX_FUSE_FRONT_DEFAULT)) {
        s.front_long(st);
        s.mask(0, fuse ? &mt : nullptr, st);
        if (!fuse)
            tail(s.list_short, s.counts + 1, fuse, st);
        return post_launch(h, what);
    }
    /* Other batches without a split (and PACX_FUSE_FRONT=0): the whole step on the caller's stream, or
       (pacx_set_side_fork) the side chain, which only reads the PCM, forked to the handle's second stream next to the transform.  The fork pays only where HIP puts
       the two streams on ONE hardware queue -- with two handles in a process it does (50.6 against 49.3 M cf/s with
       two steps in flight), with one handle it does not, and a fork and a join across hardware queues (13 + 12 us)
       cost more than the 20 us of overlap: 39.1 against 42.6 M cf/s with one step in flight */
    const bool one_stream = !h->fork_side;
    hipStream_t side_st = one_stream ? st : h->side_stream;
    if (!one_stream) {
        HIP_TRY_FORKED(h, hipEventRecord(h->ev_fork, st));
        HIP_TRY_FORKED(h, hipStreamWaitEvent(h->side_stream, h->ev_fork, 0));
    }
    s.side(0, false, side_st);
    if (!one_stream)
        HIP_TRY_FORKED(h, hipEventRecord(h->ev_join, h->side_stream));
    s.mdct(st);
    if (!one_stream)
        HIP_TRY_FORKED(h, hipStreamWaitEvent(st, h->ev_join, 0));       /* join */
    s.mask(0, fuse ? &mt : nullptr, st);
    /* what is left: the long frames when not fused, the short-coded frames of a mixed batch */
    if (!fuse || mixed)
        tail(s.list_short, s.counts + 1, fuse, st);
    return post_launch_forked(h, what);
}

extern "C" int pacx_set_side_fork(pacx_handle *h, int enable)
{
    if (!h)
        return PACX_E_ARG;
    h->fork_side = enable ? 1 : 0;
    return PACX_OK;
}

extern "C" int pacx_encode_batch(pacx_handle *h, const pacx_pcm *in, const uint8_t *frame_flags,
                                 int32_t *overall_scale, int32_t *scale_factor, int32_t *bit_alloc,
                                 int32_t *mantissa, uint32_t *status, void *stream)
{
    return encode_scalar(h, in, frame_flags, overall_scale, scale_factor, bit_alloc, mantissa, status, nullptr,
                         nullptr, stream, "pacx_encode_batch");
}

extern "C" int pacx_encode_pack_batch(pacx_handle *h, const pacx_pcm *in, const uint8_t *frame_flags,
                                      int32_t *overall_scale, int32_t *scale_factor, int32_t *bit_alloc,
                                      int32_t *mantissa, uint32_t *status, uint8_t *payload, int32_t *n_bytes,
                                      void *stream)
{
    if (h && in && in->n_frames > 0 && (!payload || !n_bytes))
        return fail(h, PACX_E_ARG, "pacx_encode_pack_batch: payload and n_bytes are required");
    return encode_scalar(h, in, frame_flags, overall_scale, scale_factor, bit_alloc, mantissa, status, payload,
                         n_bytes, stream, "pacx_encode_pack_batch");
}

extern "C" int pacx_encode_vq_batch(pacx_handle *h, const pacx_pcm *in, const uint8_t *frame_flags,
                                    int32_t *overall_scale, int32_t *bit_alloc, uint8_t *payload,
                                    int32_t *n_bytes, uint32_t *status, pacx_vq_entry *entries,
                                    int32_t *entry_count, int32_t entries_per_band, void *stream)
{
    if (!h)
        return PACX_E_ARG;
    EncodeStep s(h, frame_flags, stream);
    int rc = s.view(in);
    if (rc || s.n_cf == 0)
        return rc;
    if (!overall_scale || !bit_alloc || !payload || !n_bytes || !status)
        return fail(h, PACX_E_ARG, "pacx_encode_vq_batch: null output pointer");
    if ((entries && (!entry_count || entries_per_band < 1)) || (!entries && entry_count && entries_per_band != 0))
        return fail(h, PACX_E_ARG, "pacx_encode_vq_batch: entries need entry_count and entries_per_band >= 1");
    if ((rc = vq_only(h, "pacx_encode_vq_batch")))
        return rc;
    const PacxTables &T = h->T;
    const long long n_cf = s.n_cf;
    const int fast = s.fast, mixed = s.mixed;
    hipStream_t st = s.stream;
    if ((rc = s.reserve({mixed ? GROW_VQ_UNITS : GROW_NONE})) || (rc = s.init_outputs(overall_scale, status)))
        return rc;
    /* every long-coded frame gets its n_bytes from the coder; only dropped short hops keep the zero */
    if (mixed)
        HIP_TRY(h, hipMemsetAsync(n_bytes, 0, (size_t)n_cf * sizeof(int32_t), st));
    MaskTail mt;
    memset(&mt, 0, sizeof(mt));
    mt.bit_alloc = bit_alloc;
    mt.status = status;
    /* BitAlloc as a kernel of its own; skip_long: 0 every frame, 1 the short-coded frames only, 2 the long-coded only */
    auto bitalloc = [&](int skip_long, hipStream_t s2) {
        pacx_launch_bitalloc(T, frame_flags, s.n_ch, n_cf, 0, mixed, skip_long, h->ws_smr, bit_alloc, status, s2);
    };
    const VqCode code = {bit_alloc, status, payload, n_bytes, h->ws_sbr_mean, entries, entry_count,
                         entries ? entries_per_band : 0};
    auto vq = [&](int stage, const int32_t *cf_list, const int32_t *cf_count, hipStream_t s2) {
        s.vq(code, stage, cf_list, cf_count, s2);
    };
    const bool split = mixed && fast && h->force.split_short != 0;
    if (split) {
        /* a block-switched batch: the long-coded and the short-coded frames are two independent chains up
           to the gain-shape coder (which takes all frames), as in the scalar entry point:
             long :  k_mdct_long_v2 -> k_side_long (folds max|FFT| into the overall scale of SBR blocks) ->
                     k_mask<1024> with BitAlloc
             short:  k_mdct_short -> k_side_short -> k_mask<128> -> k_bitalloc
           side by side on two streams; the side chains and the short MDCT go by the flags alone and start
           while the frame lists are made */
        const int vq_fuse_split = h->force.vq_fuse_alloc != 0;  /* PACX_VQ_FUSE_ALLOC=0: k_bitalloc behind the mask kernel */
        HIP_TRY(h, hipEventRecord(h->ev_fork, st));
        HIP_TRY_FORKED(h, hipStreamWaitEvent(h->short_stream, h->ev_fork, 0));
        s.lists(st);
        HIP_TRY_FORKED(h, hipEventRecord(h->ev_lists, st));
        /* short chain */
        s.mdct_short(h->short_stream);
        s.side(PACX_PART_SHORT, false, h->short_stream);
        HIP_TRY_FORKED(h, hipStreamWaitEvent(h->short_stream, h->ev_lists, 0));
        s.mask(PACX_PART_SHORT, nullptr, h->short_stream);
        bitalloc(1, h->short_stream);
        /* Each chain goes on into the gain-shape coder with its own frames: two k_vq_frame launches side by side on
           the two streams (0.685 ms per shipped128 step with direct launches, against 0.74-0.77 ms for one launch
           over all frames behind the join of the two chains).  Replayed from a hipGraph the two launches do not
           overlap (0.822 ms): bench.py does not capture gain-shape steps */
        vq(1, s.list_short, s.counts + 1, h->short_stream);
        HIP_TRY_FORKED(h, hipEventRecord(h->ev_short_done, h->short_stream));
        /* long chain */
        s.mdct_long(st);
        s.side(PACX_PART_LONG, T.use_sbr, st);
        s.mask(PACX_PART_LONG, vq_fuse_split ? &mt : nullptr, st);
        if (!vq_fuse_split)       /* BitAlloc of the long frames in k_bitalloc behind the mask kernel (part 2 = long only) */
            bitalloc(2, st);
        vq(1, s.list_long, s.counts, st);
        HIP_TRY_FORKED(h, hipStreamWaitEvent(st, h->ev_short_done, 0));       /* both chains done */
    } else {
        if (mixed)
            s.lists(st);
        s.mdct(st);
        /* the side chain follows the MDCT on the same stream: with SBR it folds max|FFT| into the overall scale
           the MDCT wrote, and without SBR a fork to a second stream costs more than it hides here (0.677 against
           0.661 ms per step, A/B on one box) */
        s.side(0, T.use_sbr, st);
        /* BitAlloc of the long frames inside the mask kernel or in k_bitalloc behind it: as with the scalar
           coder's tail, all-long batches are a little faster unfused (0.637 against 0.642 ms per step, A/B on one
           box); PACX_VQ_FUSE_ALLOC=0/1 forces either */
        const int vq_fuse = h->force.vq_fuse_alloc >= 0 ? h->force.vq_fuse_alloc : mixed;
        s.mask(0, vq_fuse ? &mt : nullptr, st);
        bitalloc(vq_fuse, st);
    }
    vq(split ? 2 : 0, nullptr, nullptr, st);
    return post_launch(h, "pacx_encode_vq_batch");
}

extern "C" int pacx_pack_batch(pacx_handle *h, int64_t n_cf, int n_channels, const uint8_t *frame_flags,
                               const int32_t *overall_scale, const int32_t *scale_factor,
                               const int32_t *bit_alloc, const int32_t *mantissa, const uint32_t *status,
                               uint8_t *payload, int32_t *n_bytes, void *stream)
{
    if (!h)
        return PACX_E_ARG;
    if (n_cf == 0)
        return PACX_OK;
    if (n_cf < 0 || n_channels < 1 || !overall_scale || !scale_factor || !bit_alloc || !mantissa || !payload ||
        !n_bytes)
        return fail(h, PACX_E_ARG, "pacx_pack_batch: bad argument");
    HIP_TRY(h, hipSetDevice(h->device));
    pacx_launch_pack(h->T, frame_flags, n_channels, n_cf, overall_scale, scale_factor, bit_alloc, mantissa,
                     status, payload, PACX_PAYLOAD_STRIDE, n_bytes, (hipStream_t)stream);
    return post_launch(h, "pacx_pack_batch");
}

extern "C" int pacx_gather_body(pacx_handle *h, int64_t n_cf, const uint8_t *payload, const int32_t *n_bytes,
                                uint8_t *body, int64_t body_capacity, int64_t *total_bytes, void *stream)
{
    if (!h)
        return PACX_E_ARG;
    if (n_cf == 0) {
        if (total_bytes)
            HIP_TRY(h, hipMemsetAsync(total_bytes, 0, sizeof(int64_t), (hipStream_t)stream));
        return PACX_OK;
    }
    if (n_cf < 0 || !payload || !n_bytes || !body || body_capacity < 0)
        return fail(h, PACX_E_ARG, "pacx_gather_body: bad argument");
    HIP_TRY(h, hipSetDevice(h->device));
    int rc = pacx_reserve(h, n_cf);
    if (rc)
        return rc;
    pacx_launch_gather(n_cf, payload, PACX_PAYLOAD_STRIDE, n_bytes, h->ws_chunks, h->ws_offs, body, body_capacity,
                       (long long *)total_bytes, (hipStream_t)stream);
    return post_launch(h, "pacx_gather_body");
}

/* ---- function-level entry points (k_misc.hip) --------------------------- */
extern "C" int pacx_window_batch(pacx_handle *h, int window, int64_t n_rows, const double *x, double *y,
                                 void *stream)
{
    if (!h)
        return PACX_E_ARG;
    if (n_rows < 0 || !x || !y)
        return fail(h, PACX_E_ARG, "pacx_window_batch: bad argument");
    const double *w;
    int len;
    switch (window) {
    case PACX_WIN_SINE: case PACX_WIN_START: case PACX_WIN_STOP: case PACX_WIN_STARTSTOP:
        w = h->T.win_long + window * PACX_N_LONG; len = PACX_N_LONG; break;
    case PACX_WIN_SINE_SHORT: w = h->T.win_short; len = PACX_N_SHORT; break;
    case PACX_WIN_HANN: w = h->T.hann_long; len = PACX_N_LONG; break;
    case PACX_WIN_HANN_SHORT: w = h->T.hann_short; len = PACX_N_SHORT; break;
    case PACX_WIN_KBD: w = h->T.kbd_long; len = PACX_N_LONG; break;
    case PACX_WIN_KBD_SHORT: w = h->T.kbd_short; len = PACX_N_SHORT; break;
    default: return fail(h, PACX_E_ARG, "pacx_window_batch: unknown window");
    }
    HIP_TRY(h, hipSetDevice(h->device));
    pacx_launch_window(w, n_rows, len, x, y, (hipStream_t)stream);
    return post_launch(h, "pacx_window_batch");
}

extern "C" int pacx_window_table_batch(pacx_handle *h, const double *table, int len, int64_t n_rows,
                                       const double *x, double *y, void *stream)
{
    if (!h)
        return PACX_E_ARG;
    if (n_rows < 0 || len < 1 || !table || !x || !y)
        return fail(h, PACX_E_ARG, "pacx_window_table_batch: bad argument");
    HIP_TRY(h, hipSetDevice(h->device));
    pacx_launch_window(table, n_rows, len, x, y, (hipStream_t)stream);
    return post_launch(h, "pacx_window_table_batch");
}

static int quant_elem(pacx_handle *h, int op, int64_t n, const double *x, int scale, int a, int b,
                      int64_t *out, void *stream, const char *what)
{
    if (!h)
        return PACX_E_ARG;
    if (n < 0 || !x || !out)
        return fail(h, PACX_E_ARG, std::string(what) + ": bad argument");
    const int r_bits = (op == 0) ? a : ((1 << a) - 1 + b);
    if (a < 1 || b < 0 || r_bits < 1 || r_bits > 62 || (op >= 2 && (b < 1 || scale < 0 || scale > (1 << a) - 1)))
        return fail(h, PACX_E_UNSUPPORTED, std::string(what) + ": bit widths out of range");
    HIP_TRY(h, hipSetDevice(h->device));
    pacx_launch_quant_elem(op, n, x, scale, a, b, out, (hipStream_t)stream);
    return post_launch(h, what);
}

extern "C" int pacx_quantize_uniform(pacx_handle *h, int64_t n, const double *x, int n_bits, int64_t *codes,
                                     void *stream)
{
    return quant_elem(h, 0, n, x, 0, n_bits, 0, codes, stream, "pacx_quantize_uniform");
}

extern "C" int pacx_scale_factor(pacx_handle *h, int64_t n, const double *x, int n_scale_bits,
                                 int n_mant_bits, int64_t *scale, void *stream)
{
    return quant_elem(h, 1, n, x, 0, n_scale_bits, n_mant_bits, scale, stream, "pacx_scale_factor");
}

extern "C" int pacx_mantissa(pacx_handle *h, int64_t n, const double *x, int scale, int n_scale_bits,
                             int n_mant_bits, int64_t *mantissa, void *stream)
{
    return quant_elem(h, 2, n, x, scale, n_scale_bits, n_mant_bits, mantissa, stream, "pacx_mantissa");
}

static int dequant_elem(pacx_handle *h, int op, int64_t n, const int64_t *codes, int scale, int a, int b,
                        double *out, void *stream, const char *what)
{
    if (!h)
        return PACX_E_ARG;
    if (n < 0 || !codes || !out)
        return fail(h, PACX_E_ARG, std::string(what) + ": bad argument");
    const int r_bits = (op == 0) ? a : ((1 << a) - 1 + b);
    /* 2 * code and 2^R - 1 must be exact doubles for the one division to be the reference's value */
    if (a < 1 || b < 0 || r_bits < 1 || r_bits > 53 || (op >= 1 && (b < 1 || scale < 0 || scale > (1 << a) - 1)))
        return fail(h, PACX_E_UNSUPPORTED, std::string(what) + ": bit widths out of range");
    HIP_TRY(h, hipSetDevice(h->device));
    pacx_launch_dequant_elem(op, n, codes, scale, a, b, out, (hipStream_t)stream);
    return post_launch(h, what);
}

extern "C" int pacx_dequantize_uniform(pacx_handle *h, int64_t n, const int64_t *codes, int n_bits, double *x,
                                       void *stream)
{
    return dequant_elem(h, 0, n, codes, 0, n_bits, 0, x, stream, "pacx_dequantize_uniform");
}

extern "C" int pacx_dequantize(pacx_handle *h, int64_t n, const int64_t *mantissa, int scale, int n_scale_bits,
                               int n_mant_bits, double *x, void *stream)
{
    return dequant_elem(h, 1, n, mantissa, scale, n_scale_bits, n_mant_bits, x, stream, "pacx_dequantize");
}

extern "C" int pacx_mantissa_fp(pacx_handle *h, int64_t n, const double *x, int scale, int n_scale_bits,
                                int n_mant_bits, int64_t *mantissa, void *stream)
{
    return quant_elem(h, 3, n, x, scale, n_scale_bits, n_mant_bits, mantissa, stream, "pacx_mantissa_fp");
}

extern "C" int pacx_dequantize_fp(pacx_handle *h, int64_t n, const int64_t *mantissa, int scale, int n_scale_bits,
                                  int n_mant_bits, double *x, void *stream)
{
    return dequant_elem(h, 2, n, mantissa, scale, n_scale_bits, n_mant_bits, x, stream, "pacx_dequantize_fp");
}

extern "C" int pacx_imdct_batch(pacx_handle *h, int64_t n_rows, int mode, const double *lines, double *blocks,
                                void *stream)
{
    if (!h)
        return PACX_E_ARG;
    if (n_rows == 0)
        return PACX_OK;
    if (n_rows < 0 || n_rows > 0x7fffffffLL || !lines || !blocks || (mode & ~PACX_MDCT_SHORT))
        return fail(h, PACX_E_ARG, "pacx_imdct_batch: bad argument");
    HIP_TRY(h, hipSetDevice(h->device));
    pacx_launch_imdct_plain(h->T, n_rows, (mode & PACX_MDCT_SHORT) ? 1 : 0, lines, blocks, (hipStream_t)stream);
    return post_launch(h, "pacx_imdct_batch");
}

extern "C" int pacx_mdct_direct_batch(pacx_handle *h, int64_t n_rows, int a, int b, int inverse, const double *x,
                                      double *y, void *stream)
{
    if (!h)
        return PACX_E_ARG;
    if (n_rows == 0)
        return PACX_OK;
    if (n_rows < 0 || !x || !y || a < 1 || b < 1 || ((a + b) & 1))
        return fail(h, PACX_E_ARG, "pacx_mdct_direct_batch: bad argument (a, b >= 1, a + b even)");
    if (a + b > 16384 || n_rows * (long long)(a + b) > 0x7fffffffLL * 128)
        return fail(h, PACX_E_UNSUPPORTED, "pacx_mdct_direct_batch: block longer than 16384 samples");
    HIP_TRY(h, hipSetDevice(h->device));
    pacx_launch_mdct_direct(n_rows, a, b, inverse ? 1 : 0, x, y, (hipStream_t)stream);
    return post_launch(h, "pacx_mdct_direct_batch");
}

extern "C" int pacx_bitalloc_generic(pacx_handle *h, int64_t n, int n_bands, const int32_t *band_lines,
                                     const double *budget, int max_mant_bits, const double *smr,
                                     int32_t *bit_alloc, void *stream)
{
    if (!h)
        return PACX_E_ARG;
    if (n < 0 || n_bands < 1 || n_bands > PACX_MAX_BANDS || !band_lines || !budget || !smr || !bit_alloc)
        return fail(h, PACX_E_ARG, "pacx_bitalloc_generic: bad argument (at most 32 bands)");
    HIP_TRY(h, hipSetDevice(h->device));
    pacx_launch_bitalloc_generic(n, n_bands, band_lines, budget, max_mant_bits, smr, bit_alloc,
                                 (hipStream_t)stream);
    return post_launch(h, "pacx_bitalloc_generic");
}

extern "C" int pacx_transient_flags(pacx_handle *h, const pacx_pcm *hops, uint8_t *transient,
                                    uint8_t *frame_flags, void *stream)
{
    if (!h)
        return PACX_E_ARG;
    EncodeStep s(h, nullptr, stream);
    const int rc = s.view(hops);
    if (rc)
        return rc;
    if (hops->dtype != PACX_PCM_I16 || !transient)
        return fail(h, PACX_E_ARG, "pacx_transient_flags: int16 hops and a transient buffer are required");
    if (hops->n_channels > 8)
        return fail(h, PACX_E_UNSUPPORTED, "pacx_transient_flags: at most 8 channels");
    HIP_TRY(h, hipSetDevice(h->device));
    pacx_launch_transient(s.v, hops->n_frames, PACX_M_LONG, transient, frame_flags, s.stream);
    return post_launch(h, "pacx_transient_flags");
}

/* ---- decode side (k_decode.hip) ------------------------------------------ */
extern "C" int pacx_transient_detect_f64(pacx_handle *h, int64_t n_blocks, int n_channels, int n_samples,
                                         const double *blocks, double thresh, uint8_t *result, void *stream)
{
    if (!h)
        return PACX_E_ARG;
    if (n_blocks == 0)
        return PACX_OK;
    if (n_blocks < 0 || n_blocks > 0x7fffffffLL || n_channels < 1 || n_samples < 1 || !blocks || !result)
        return fail(h, PACX_E_ARG, "pacx_transient_detect_f64: bad argument");
    if ((long long)n_channels * n_samples > PACX_NP_SUM_MAX_N)      /* the mean indexes its elements with ints */
        return fail(h, PACX_E_UNSUPPORTED, "pacx_transient_detect_f64: block too large");
    HIP_TRY(h, hipSetDevice(h->device));
    pacx_launch_transient_f64(n_blocks, n_channels, n_samples, blocks, thresh, result, (hipStream_t)stream);
    return post_launch(h, "pacx_transient_detect_f64");
}

extern "C" int pacx_unpack_batch(pacx_handle *h, int64_t n_cf, const uint8_t *payload, int payload_stride,
                                 const int64_t *offsets, const int32_t *n_bytes, uint8_t *cf_flags,
                                 int32_t *overall_scale, int32_t *scale_factor, int32_t *bit_alloc,
                                 int32_t *mantissa, uint32_t *status, void *stream)
{
    if (!h)
        return PACX_E_ARG;
    if (n_cf == 0)
        return PACX_OK;
    if (n_cf < 0 || !payload || !n_bytes || !cf_flags || !overall_scale || !scale_factor || !bit_alloc ||
        !mantissa || (!offsets && payload_stride <= 0))
        return fail(h, PACX_E_ARG, "pacx_unpack_batch: bad argument");
    HIP_TRY(h, hipSetDevice(h->device));
    pacx_launch_unpack(h->T, n_cf, payload, payload_stride, (const long long *)offsets, n_bytes, cf_flags,
                       overall_scale, scale_factor, bit_alloc, mantissa, status, (hipStream_t)stream);
    return post_launch(h, "pacx_unpack_batch");
}

/* where pacx_launch_decode leaves the windowed blocks: the caller's array, else the handle's when only PCM is wanted */
static int decode_work(pacx_handle *h, long long n_cf, double *blocks, const int16_t *pcm, double **work)
{
    *work = blocks;
    if (!blocks && pcm && n_cf > 0) {
        const int rc = grow(h, GROW_DEC_BLOCKS, n_cf);
        if (rc != PACX_OK)
            return rc;
        *work = h->ws_blocks;
    }
    return PACX_OK;
}

static int decode_scalar(pacx_handle *h, const char *what, int64_t n_blocks, int n_channels, const uint8_t *cf_flags,
                         const int32_t *overall_scale, const int32_t *scale_factor, const int32_t *bit_alloc,
                         const int32_t *mantissa, double *lines, double *blocks, int16_t *pcm, uint32_t *status,
                         int routing, void *stream)
{
    if (!h)
        return PACX_E_ARG;
    if (routing < 0 || routing > 2 || n_blocks < 0 || n_channels < 1 || (n_blocks > 0 && (!cf_flags || !overall_scale || !scale_factor ||
                                                              !bit_alloc || !mantissa)) ||
        (!blocks && !pcm && !lines))
        return fail(h, PACX_E_ARG, std::string(what) + ": bad argument");
    if (int rc = not_vq(h, what, "pacx_decode_vq_batch reads gain-shape streams"))
        return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    hipStream_t st = (hipStream_t)stream;
    const long long n_cf = n_blocks * n_channels;
    double *work;
    if (int rc = decode_work(h, n_cf, blocks, pcm, &work))
        return rc;
    const double *lines_in = nullptr;
    if (!h->T.use_sbr)
        routing = 0;
    if (n_cf > 0 && (routing || lines)) {
        /* an SBR file (PACFile.Decode, coder/pacfile.py:645-668: long blocks with a coded omitted band are
           Decode_SBR's, coder/codec.py:95-222 scalar branch), or a caller who wants the dequantised lines */
        const int rc = grow(h, GROW_DEC_LINES, n_cf);
        if (rc != PACX_OK)
            return rc;
        double *ln = lines ? lines : h->ws_dec_lines;
        uint32_t *stw = status ? status : h->ws_dec_status;
        HIP_TRY(h, hipMemsetAsync(stw, 0, (size_t)n_cf * sizeof(uint32_t), st));
        pacx_launch_sbr_scalar_lines(h->T, n_cf, cf_flags, scale_factor, bit_alloc, mantissa, ln, h->ws_dec_sbr, routing,
                                     st);
        if (routing)
            pacx_launch_sbr_recon(h->T, h->vqdec_view.data(), n_cf, h->ws_dec_sbr, ln, stw, st);
        lines_in = ln;
    } else if (status && n_cf > 0) {
        HIP_TRY(h, hipMemsetAsync(status, 0, (size_t)n_cf * sizeof(uint32_t), st));
    }
    if (work || pcm)
        pacx_launch_decode(h->T, n_blocks, n_channels, cf_flags, overall_scale, scale_factor, bit_alloc, mantissa,
                           lines_in, work, pcm, st);
    return post_launch(h, what);
}

extern "C" int pacx_decode_batch(pacx_handle *h, int64_t n_blocks, int n_channels, const uint8_t *cf_flags,
                                 const int32_t *overall_scale, const int32_t *scale_factor,
                                 const int32_t *bit_alloc, const int32_t *mantissa, double *blocks,
                                 int16_t *pcm, void *stream)
{
    if (h && !blocks && !pcm)
        return fail(h, PACX_E_ARG, "pacx_decode_batch: bad argument");
    return decode_scalar(h, "pacx_decode_batch", n_blocks, n_channels, cf_flags, overall_scale, scale_factor, bit_alloc,
                         mantissa, nullptr, blocks, pcm, nullptr, 0, stream);
}

extern "C" int pacx_decode_sbr_batch(pacx_handle *h, int64_t n_blocks, int n_channels, const uint8_t *cf_flags,
                                     const int32_t *overall_scale, const int32_t *scale_factor,
                                     const int32_t *bit_alloc, const int32_t *mantissa, int routing,
                                     double *lines, double *blocks, int16_t *pcm, uint32_t *status, void *stream)
{
    return decode_scalar(h, "pacx_decode_sbr_batch", n_blocks, n_channels, cf_flags, overall_scale, scale_factor,
                         bit_alloc, mantissa, lines, blocks, pcm, status, routing ? 2 : 1, stream);
}

extern "C" int pacx_decode_vq_batch(pacx_handle *h, int64_t n_blocks, int n_channels, const uint8_t *payload,
                                    int payload_stride, const int64_t *offsets, const int32_t *n_bytes,
                                    uint8_t *cf_flags, int32_t *overall_scale, int32_t *bit_alloc,
                                    double *lines, double *blocks, int16_t *pcm, uint32_t *status,
                                    void *stream)
{
    if (!h)
        return PACX_E_ARG;
    if (n_blocks < 0 || n_channels < 1 ||
        (n_blocks > 0 && (!payload || !n_bytes || !cf_flags || !overall_scale || !bit_alloc || !status ||
                          (!offsets && payload_stride <= 0))))
        return fail(h, PACX_E_ARG, "pacx_decode_vq_batch: bad argument");
    if (int rc = vq_only(h, "pacx_decode_vq_batch"))
        return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    const long long n_cf = n_blocks * n_channels;
    hipStream_t st = (hipStream_t)stream;
    {
        const int rc = grow(h, GROW_DEC_LINES, n_cf);
        if (rc != PACX_OK)
            return rc;
    }
    double *ln = lines ? lines : h->ws_dec_lines;
    double *work;
    if (int rc = decode_work(h, n_cf, blocks, pcm, &work))
        return rc;
    if (n_cf > 0) {
        HIP_TRY(h, hipMemsetAsync(status, 0, (size_t)n_cf * sizeof(uint32_t), st));
        pacx_launch_vq_dec(h->T, h->vqdec_view.data(), n_cf, payload, payload_stride, (const long long *)offsets,
                           n_bytes, cf_flags, overall_scale, bit_alloc, ln, h->ws_dec_sbr, status, h->force.vq_dec_frame,
                           st);
    }
    if (work || pcm)
        pacx_launch_decode(h->T, n_blocks, n_channels, cf_flags, overall_scale, nullptr, nullptr, nullptr, ln,
                           work, pcm, st);
    return post_launch(h, "pacx_decode_vq_batch");
}

/* ---- decoding a stream in chunks: where the records start, and the half-block across a chunk boundary ---- */
extern "C" int pacx_index_body(pacx_handle *h, const uint8_t *body, int64_t n_body, int n_channels, int final,
                               int64_t max_records, int64_t *offsets, int32_t *n_bytes, int64_t *result, void *stream)
{
    if (!h)
        return PACX_E_ARG;
    if (n_body < 0 || n_channels < 1 || max_records < 0 || !result || (n_body > 0 && !body) ||
        (max_records > 0 && (!offsets || !n_bytes)))
        return fail(h, PACX_E_ARG, "pacx_index_body: bad argument");
    if (n_body / PACX_IX_SEG + 1 > 0x7FFFFFFFll)
        return fail(h, PACX_E_UNSUPPORTED, "pacx_index_body: body too long for one call");
    HIP_TRY(h, hipSetDevice(h->device));
    PacxIndexWs ws;
    const int rc = grow(h, GROW_INDEX, (long long)pacx_index_ws_bytes(n_body, &ws));
    if (rc)
        return rc;
    pacx_launch_index(ws, h->ws_index, body, n_body, n_channels, final != 0, max_records, (long long *)offsets, n_bytes,
                      (long long *)result, (hipStream_t)stream);
    return post_launch(h, "pacx_index_body");
}

extern "C" int pacx_overlap_add_pcm(pacx_handle *h, int64_t n_blocks, int n_channels, const double *blocks, double *tail,
                                    int flush, int16_t *pcm, void *stream)
{
    if (!h)
        return PACX_E_ARG;
    if (n_blocks < 0 || n_channels < 1 || !tail || (n_blocks > 0 && !blocks) || ((n_blocks > 0 || flush) && !pcm))
        return fail(h, PACX_E_ARG, "pacx_overlap_add_pcm: bad argument");
    HIP_TRY(h, hipSetDevice(h->device));
    pacx_launch_ola_tail(n_blocks, n_channels, blocks, tail, flush != 0, pcm, (hipStream_t)stream);
    return post_launch(h, "pacx_overlap_add_pcm");
}

/* ---- quality of an encode: noise-to-mask ratios ---- */
extern "C" int pacx_nmr_batch(pacx_handle *h, const pacx_pcm *in, const uint8_t *frame_flags, const double *dec_lines,
                              const int32_t *overall_scale, const uint32_t *status, double *noise, double *mask,
                              double *nmr_db, void *stream)
{
    if (!h)
        return PACX_E_ARG;
    EncodeStep s(h, frame_flags, stream);
    int rc = s.view(in);
    if (rc || s.n_cf == 0)
        return rc;
    if (!dec_lines || !overall_scale || !noise || !mask || !nmr_db)
        return fail(h, PACX_E_ARG, "pacx_nmr_batch: null pointer");
    if ((rc = s.reserve({GROW_NMR})))
        return rc;
    hipStream_t st = s.stream;
    /* the encoder's own front end on one stream: the original's lines in ws_lines (its overall scales go to the
       workspace as they come and are not used: the noise is taken against the scales the decoder read; no status
       words), the maskers, then the masked threshold of every line */
    s.overall_scale = h->ws_overall;
    s.front(h->ws_thr, st);
    pacx_launch_nmr(h->T, frame_flags, s.n_ch, s.n_cf, h->ws_lines, dec_lines, overall_scale, h->ws_thr, status, noise, mask,
                    nmr_db, st);
    return post_launch(h, "pacx_nmr_batch");
}

/* ---- coding to a target noise-to-mask ratio ---- */
/* the front end of pacx_nmr_batch on one stream (lines, SMRs and, for the search, the threshold of every line), the
   allocation by k_rate_search or from the caller's budgets, then the separate-kernel chain k_quantize -> k_pack.
   With the caller's allocation (ALLOC_GIVEN) the front end is the MDCT alone: nothing here reads SMRs or maskers. */
enum { BUDGET_SEARCH, BUDGET_GIVEN, ALLOC_GIVEN };
static int encode_budgeted(pacx_handle *h, const pacx_pcm *in, const uint8_t *frame_flags, int mode,
                           double target_nmr_db, double max_bits_per_sample, const int32_t *budget_in,
                           const int32_t *alloc_in, int32_t *overall_scale, int32_t *scale_factor, int32_t *bit_alloc, int32_t *mantissa,
                           uint32_t *status, uint8_t *payload, int32_t *n_bytes, int32_t *budget_out, void *stream,
                           const char *what)
{
    if (!h)
        return PACX_E_ARG;
    int rc = scalar_only(h, what);
    if (rc)
        return rc;
    const bool search = mode == BUDGET_SEARCH, given = mode == ALLOC_GIVEN;
    if (search && !std::isfinite(target_nmr_db))
        return fail(h, PACX_E_ARG, std::string(what) + ": target_nmr_db is not finite");
    EncodeStep s(h, frame_flags, stream);
    if ((search && (rc = check_cap_rate(h, what, max_bits_per_sample))) || (rc = s.view(in)))
        return rc;
    if (!overall_scale || !scale_factor || !bit_alloc || !status || !payload || !n_bytes ||
        (search ? !budget_out : given ? !alloc_in : !budget_in))
        return fail(h, PACX_E_ARG, std::string(what) + ": null pointer");
    if (s.n_cf == 0)
        return PACX_OK;
    /* without the caller's mantissa array the workspace's: k_pack reads the mantissas back from memory */
    if ((rc = s.reserve({search ? GROW_NMR : GROW_NONE, mantissa ? GROW_NONE : GROW_MANT})))
        return rc;
    if (!mantissa)
        mantissa = h->ws_mant;
    if ((rc = s.init_outputs(overall_scale, status)))
        return rc;
    const long long n_cf = s.n_cf;
    hipStream_t st = s.stream;
    if (given) {
        if (s.mixed)
            s.lists(st);
        s.mdct(st);
    } else {
        s.front(search ? h->ws_thr : nullptr, st);
    }
    if (given)
        pacx_launch_band_sanitize(h->T, frame_flags, s.n_ch, n_cf, alloc_in, bit_alloc, status, PACX_PAYLOAD_STRIDE, st);
    else if (search)
        pacx_launch_rate_search(h->T, frame_flags, s.n_ch, n_cf, target_nmr_db, max_bits_per_sample, h->ws_lines,
                                h->ws_thr, h->ws_smr, overall_scale, budget_out, bit_alloc, status, st);
    else
        pacx_launch_bitalloc_budget(h->T, frame_flags, s.n_ch, n_cf, budget_in, h->ws_smr, bit_alloc, status, st);
    pacx_launch_quantize(h->T, frame_flags, s.n_ch, n_cf, 0, s.mixed, h->ws_lines, overall_scale, PACX_SUB, bit_alloc,
                         scale_factor, mantissa, st);
    pacx_launch_pack(h->T, frame_flags, s.n_ch, n_cf, overall_scale, scale_factor, bit_alloc, mantissa, status, payload,
                     PACX_PAYLOAD_STRIDE, n_bytes, st);
    return post_launch(h, what);
}

extern "C" int pacx_encode_pack_nmr_batch(pacx_handle *h, const pacx_pcm *in, const uint8_t *frame_flags,
                                          double target_nmr_db, double max_bits_per_sample, int32_t *overall_scale,
                                          int32_t *scale_factor, int32_t *bit_alloc, int32_t *mantissa, uint32_t *status,
                                          uint8_t *payload, int32_t *n_bytes, int32_t *budget, void *stream)
{
    return encode_budgeted(h, in, frame_flags, BUDGET_SEARCH, target_nmr_db, max_bits_per_sample, nullptr, nullptr, overall_scale,
                           scale_factor, bit_alloc, mantissa, status, payload, n_bytes, budget, stream,
                           "pacx_encode_pack_nmr_batch");
}

extern "C" int pacx_encode_pack_budget_batch(pacx_handle *h, const pacx_pcm *in, const uint8_t *frame_flags,
                                             const int32_t *budget, int32_t *overall_scale, int32_t *scale_factor,
                                             int32_t *bit_alloc, int32_t *mantissa, uint32_t *status, uint8_t *payload,
                                             int32_t *n_bytes, void *stream)
{
    return encode_budgeted(h, in, frame_flags, BUDGET_GIVEN, 0.0, 0.0, budget, nullptr, overall_scale, scale_factor, bit_alloc,
                           mantissa, status, payload, n_bytes, nullptr, stream, "pacx_encode_pack_budget_batch");
}

extern "C" int pacx_encode_pack_alloc_batch(pacx_handle *h, const pacx_pcm *in, const uint8_t *frame_flags,
                                            const int32_t *bit_alloc_in, int32_t *overall_scale, int32_t *scale_factor,
                                            int32_t *bit_alloc, int32_t *mantissa, uint32_t *status, uint8_t *payload,
                                            int32_t *n_bytes, void *stream)
{
    return encode_budgeted(h, in, frame_flags, ALLOC_GIVEN, 0.0, 0.0, nullptr, bit_alloc_in, overall_scale, scale_factor,
                           bit_alloc, mantissa, status, payload, n_bytes, nullptr, stream, "pacx_encode_pack_alloc_batch");
}

/* ---- coding to an average bit rate: the curve of every unit, then one target for the stream ---- */
/* row and sub_stride of a curve: J + 1 of the widest long block, eight times J + 1 of the widest short sub-block */
static void rate_curve_layout(const PacxTables &T, double max_bps, int *row, int *sub_stride)
{
    int j_long = 0, j_short = 0;
    for (int lon = 0; lon < 2; ++lon) {
        const int jl = pacx_rate_steps(max_bps, PACX_M_LONG, 0, lon, T.n_scale_bits, T.n_mant_size_bits, T.nb_long);
        const int js = pacx_rate_steps(max_bps, PACX_M_SHORT, 1, lon, T.n_scale_bits, T.n_mant_size_bits, T.nb_short);
        j_long = jl > j_long ? jl : j_long;
        j_short = js > j_short ? js : j_short;
    }
    *sub_stride = j_short + 1;
    *row = j_long + 1 > PACX_SUB * (j_short + 1) ? j_long + 1 : PACX_SUB * (j_short + 1);
}

extern "C" int pacx_rate_curve_layout(const pacx_handle *h, double max_bits_per_sample, int32_t *row,
                                      int32_t *sub_stride)
{
    if (!h || !row || !sub_stride)
        return PACX_E_ARG;
    if (h->T.use_vq || h->T.use_sbr)
        return PACX_E_UNSUPPORTED;
    if (!cap_rate_ok(max_bits_per_sample))
        return PACX_E_ARG;
    int r, s;
    rate_curve_layout(h->T, max_bits_per_sample, &r, &s);
    *row = r;
    *sub_stride = s;
    return PACX_OK;
}

/* the longest record a pick can give at this cap rate, in bytes: per unit the header bits and at most
   min(32 J, maxMantBits x lines) mantissa bits (a unit within its cap, or BitAlloc's at that budget) */
static long long band_record_bound(const PacxTables &T, double max_bps)
{
    int max_mant = 1 << T.n_mant_size_bits;
    if (max_mant > 16)
        max_mant = 16;
    long long worst = 0;
    for (int sh = 0; sh < 2; ++sh)
        for (int lon = 0; lon < 2; ++lon) {
            const int nb = sh ? T.nb_short : T.nb_long, m = sh ? PACX_M_SHORT : PACX_M_LONG;
            const long long all = (long long)max_mant * m;
            const long long j = pacx_rate_steps(max_bps, m, sh, lon, T.n_scale_bits, T.n_mant_size_bits, nb);
            const long long mant = 32 * j < all ? 32 * j : all;
            const long long bytes = record_bytes(T.n_scale_bits, T.n_mant_size_bits, nb, mant, sh != 0);
            worst = bytes > worst ? bytes : worst;
        }
    return worst;
}

/* pacx_rate_curve_batch and pacx_band_curve_batch: the checks and the front end of pacx_encode_pack_nmr_batch (overall
   scales and status words stay in the workspace), then the curve kernel of one of them.  band: nmr, cap, cap_alloc;
   else worst, bits, steps with rows of `row` */
static int curve_batch(pacx_handle *h, bool band, const char *what, const pacx_pcm *in, const uint8_t *frame_flags,
                       double max_bits_per_sample, int32_t row, double *curve, int32_t *a, int32_t *b, void *stream)
{
    if (!h)
        return PACX_E_ARG;
    EncodeStep s(h, frame_flags, stream);
    int rc;
    if ((rc = scalar_only(h, what)) || (rc = check_cap_rate(h, what, max_bits_per_sample)) || (rc = s.view(in)))
        return rc;
    if (!curve || !a || !b)
        return fail(h, PACX_E_ARG, std::string(what) + ": null pointer");
    int need = 0, sub_stride = 0;
    if (band) {
        if (band_record_bound(h->T, max_bits_per_sample) > PACX_PAYLOAD_STRIDE)
            return fail(h, PACX_E_UNSUPPORTED, std::string(what) + ": a record at this cap rate would not fit pacx_payload_stride");
    } else {
        rate_curve_layout(h->T, max_bits_per_sample, &need, &sub_stride);
        if (row < need)
            return fail(h, PACX_E_ARG, std::string(what) + ": row is smaller than pacx_rate_curve_layout's (" +
                                           std::to_string(need) + ")");
    }
    if (s.n_cf == 0)
        return PACX_OK;
    if ((rc = s.reserve({GROW_NMR})) || (rc = s.init_outputs(h->ws_overall, h->ws_rate_status)))
        return rc;
    const long long n_cf = s.n_cf;
    hipStream_t st = s.stream;
    s.front(h->ws_thr, st);
    if (band)
        pacx_launch_band_curve(h->T, frame_flags, s.n_ch, n_cf, max_bits_per_sample, h->ws_lines, h->ws_thr, h->ws_smr,
                               h->ws_overall, h->ws_rate_status, curve, a, b, st);
    else
        pacx_launch_rate_curve(h->T, frame_flags, s.n_ch, n_cf, max_bits_per_sample, row, sub_stride, h->ws_lines,
                               h->ws_thr, h->ws_smr, h->ws_overall, h->ws_rate_status, curve, a, b, st);
    return post_launch(h, what);
}

extern "C" int pacx_rate_curve_batch(pacx_handle *h, const pacx_pcm *in, const uint8_t *frame_flags,
                                     double max_bits_per_sample, int32_t row, double *worst, int32_t *bits,
                                     int32_t *steps, void *stream)
{
    return curve_batch(h, false, "pacx_rate_curve_batch", in, frame_flags, max_bits_per_sample, row, worst, bits, steps,
                       stream);
}

extern "C" int pacx_band_curve_batch(pacx_handle *h, const pacx_pcm *in, const uint8_t *frame_flags,
                                     double max_bits_per_sample, double *nmr, int32_t *cap, int32_t *cap_alloc,
                                     void *stream)
{
    return curve_batch(h, true, "pacx_band_curve_batch", in, frame_flags, max_bits_per_sample, 0, nmr, cap, cap_alloc,
                       stream);
}

/* ---- the band curve of the gain-shape coder, and its second pass ---- */
extern "C" int pacx_vq_band_curve_batch(pacx_handle *h, const pacx_pcm *in, const uint8_t *frame_flags,
                                        double max_bits_per_sample, double *nmr, int32_t *cap, int32_t *cap_alloc,
                                        void *stream)
{
    const char *what = "pacx_vq_band_curve_batch";
    if (!h)
        return PACX_E_ARG;
    EncodeStep s(h, frame_flags, stream);
    int rc;
    if ((rc = vq_plain_only(h, what)) || (rc = check_cap_rate(h, what, max_bits_per_sample)) || (rc = s.view(in)))
        return rc;
    if (band_record_bound(h->T, max_bits_per_sample) > PACX_PAYLOAD_STRIDE)
        return fail(h, PACX_E_UNSUPPORTED, std::string(what) + ": a record at this cap rate would not fit pacx_payload_stride");
    if (s.n_cf == 0)                           /* nothing to write: the outputs may be null, as for pacx_encode_vq_batch */
        return PACX_OK;
    if (!nmr || !cap || !cap_alloc)
        return fail(h, PACX_E_ARG, std::string(what) + ": null pointer");
    /* the overall scales and the status words of the front end stay in the workspace, as pacx_band_curve_batch keeps
       them */
    if ((rc = s.reserve({GROW_NMR, GROW_DEC_LINES, GROW_VQ_BAND, s.mixed ? GROW_VQ_UNITS : GROW_NONE})) ||
        (rc = s.init_outputs(h->ws_overall, h->ws_rate_status)))
        return rc;
    VqBandWs w;
    vq_band_ws(h->T, h->ws_vqb, h->ws_vqb_cf, &w);
    const long long n_cf = s.n_cf;
    hipStream_t st = s.stream;
    const PacxTables &T = h->T;
    /* the front end once, as pacx_encode_vq_batch runs it up to BitAlloc: lines, SMRs, the threshold of every line */
    s.front(h->ws_thr, st);
    /* cap and cap_alloc: BitAlloc at the cap budget of every unit (its status bits beside the front end's) */
    pacx_launch_vq_band_cap(T, frame_flags, s.n_ch, n_cf, max_bits_per_sample, h->ws_rate_status, cap, w.budget, st);
    pacx_launch_bitalloc_budget(T, frame_flags, s.n_ch, n_cf, w.budget, h->ws_smr, cap_alloc, h->ws_rate_status, st);
    /* a dropped hop keeps n_bytes = 0 through every pass: the coder leaves it alone, the decoder reads nothing */
    HIP_TRY(h, hipMemsetAsync(w.n_bytes, 0, (size_t)n_cf * sizeof(int32_t), st));
    /* candidate 0 is the decode of nothing */
    HIP_TRY(h, hipMemsetAsync(h->ws_dec_lines, 0, (size_t)n_cf * PACX_M_LONG * sizeof(double), st));
    int n_cand = 1 << T.n_mant_size_bits;
    if (n_cand > PACX_BAND_CAND)
        n_cand = PACX_BAND_CAND;
    const VqCode pass = {w.alloc, w.status, w.payload, w.n_bytes, nullptr, nullptr, nullptr, 0};
    for (int i = 1; i < n_cand; ++i) {             /* n_cand >= 2: there is a first pass */
        pacx_launch_vq_band_fill(T, n_cf, i + 1, h->ws_rate_status, w.alloc, w.status, st);
        s.vq(pass, 0, nullptr, nullptr, st);
        if (i == 1) {
            /* the first pass has told which bands code nothing (the coder drops them to 0 bits): candidate 0, with
               the lines of zeros still in place, and cap_alloc can be finished */
            pacx_launch_nmr(T, frame_flags, s.n_ch, n_cf, h->ws_lines, h->ws_dec_lines, h->ws_overall, h->ws_thr, nullptr,
                            w.noise, w.mask, w.nmr, st);
            pacx_launch_vq_band_store(T, frame_flags, s.n_ch, n_cf, 0, w.nmr, w.alloc, h->ws_rate_status, nullptr, nmr, st);
            pacx_launch_vq_band_zero(T, frame_flags, s.n_ch, n_cf, w.alloc, h->ws_rate_status, cap_alloc, st);
        }
        HIP_TRY(h, hipMemsetAsync(h->ws_dec_status, 0, (size_t)n_cf * sizeof(uint32_t), st));
        pacx_launch_vq_dec(T, h->vqdec_view.data(), n_cf, w.payload, PACX_PAYLOAD_STRIDE, nullptr, w.n_bytes, w.cf_flags,
                           w.dec_overall, w.dec_alloc, h->ws_dec_lines, h->ws_dec_sbr, h->ws_dec_status,
                           h->force.vq_dec_frame, st);
        pacx_launch_nmr(T, frame_flags, s.n_ch, n_cf, h->ws_lines, h->ws_dec_lines, w.dec_overall, h->ws_thr, nullptr,
                        w.noise, w.mask, w.nmr, st);
        pacx_launch_vq_band_store(T, frame_flags, s.n_ch, n_cf, i, w.nmr, w.alloc, h->ws_rate_status, w.status, nmr, st);
    }
    return post_launch(h, what);
}

extern "C" int pacx_encode_vq_alloc_batch(pacx_handle *h, const pacx_pcm *in, const uint8_t *frame_flags,
                                          const int32_t *bit_alloc_in, int32_t *overall_scale, int32_t *bit_alloc,
                                          uint8_t *payload, int32_t *n_bytes, uint32_t *status, void *stream)
{
    const char *what = "pacx_encode_vq_alloc_batch";
    if (!h)
        return PACX_E_ARG;
    EncodeStep s(h, frame_flags, stream);
    int rc;
    if ((rc = vq_plain_only(h, what)) || (rc = s.view(in)) || s.n_cf == 0)
        return rc;
    if (!bit_alloc_in || !overall_scale || !bit_alloc || !payload || !n_bytes || !status)
        return fail(h, PACX_E_ARG, std::string(what) + ": null pointer");
    if ((rc = s.reserve({s.mixed ? GROW_VQ_UNITS : GROW_NONE})) || (rc = s.init_outputs(overall_scale, status)))
        return rc;
    const long long n_cf = s.n_cf;
    hipStream_t st = s.stream;
    if (s.mixed)                               /* only dropped short hops keep the zero, as in pacx_encode_vq_batch */
        HIP_TRY(h, hipMemsetAsync(n_bytes, 0, (size_t)n_cf * sizeof(int32_t), st));
    /* the MDCT alone: nothing here reads SMRs or maskers */
    if (s.mixed)
        s.lists(st);
    s.mdct(st);
    pacx_launch_band_sanitize(h->T, frame_flags, s.n_ch, n_cf, bit_alloc_in, bit_alloc, status, PACX_PAYLOAD_STRIDE, st);
    s.vq({bit_alloc, status, payload, n_bytes, nullptr, nullptr, nullptr, 0}, 0, nullptr, nullptr, st);
    return post_launch(h, what);
}

/* ---- the solves: the target range on the grid, the segments of the segmented ones, the one checked path ---- */
static int solve_range(pacx_handle *h, const char *what, double nmr_lo_db, double nmr_hi_db, int *t_lo, int *t_hi)
{
    const double bound = 1048576.0;
    if (!std::isfinite(nmr_lo_db) || !std::isfinite(nmr_hi_db) || fabs(nmr_lo_db) > bound || fabs(nmr_hi_db) > bound)
        return fail(h, PACX_E_ARG, std::string(what) + ": target bounds must be finite (at most 2^20 dB in magnitude)");
    const double lo64 = nmr_lo_db * PACX_RATE_TARGET_GRID, hi64 = nmr_hi_db * PACX_RATE_TARGET_GRID;
    if (lo64 != floor(lo64) || hi64 != floor(hi64))
        return fail(h, PACX_E_ARG, std::string(what) + ": target bounds must be multiples of 1/64 dB");
    if (lo64 > hi64)
        return fail(h, PACX_E_ARG, std::string(what) + ": nmr_lo_db is above nmr_hi_db");
    *t_lo = (int)lo64;
    *t_hi = (int)hi64;
    return PACX_OK;
}

/* the host arrays of a segmented solve (include/pacx.h, pacx_rate_solve_segments) */
static int check_segments(pacx_handle *h, const char *what, int64_t n_cf, int64_t n_seg, const int64_t *seg_first,
                          const int64_t *limit_bytes)
{
    if (n_seg < 1 || n_seg > 0x7fffffffLL / PACX_SUB)
        return fail(h, PACX_E_ARG, std::string(what) + ": bad segment count");
    if (!seg_first || !limit_bytes)
        return fail(h, PACX_E_ARG, std::string(what) + ": null pointer");
    if (seg_first[0] != 0 || seg_first[n_seg] != n_cf)
        return fail(h, PACX_E_ARG, std::string(what) + ": seg_first must run from 0 to n_cf");
    for (int64_t s = 0; s < n_seg; ++s) {
        if (seg_first[s + 1] < seg_first[s])
            return fail(h, PACX_E_ARG, std::string(what) + ": seg_first decreases at segment " + std::to_string(s));
        if (limit_bytes[s] < 0)
            return fail(h, PACX_E_ARG, std::string(what) + ": negative limit for segment " + std::to_string(s));
    }
    return PACX_OK;
}

/* room for n_seg + more_states states, and the boundaries and limits in ws_seg: copied to the pinned staging buffer
   before this returns (the caller's arrays are free again), from there on `st`.  The staging buffer is the handle's
   one, so the upload before this one is waited for first; it has long run unless the caller queues segmented solves
   back to back. */
static int upload_segments(pacx_handle *h, int64_t n_seg, const int64_t *seg_first, const int64_t *limit_bytes,
                           int64_t more_states, hipStream_t st)
{
    int rc = grow(h, GROW_SOLVE, n_seg + more_states);
    if (rc)
        return rc;
    if (!h->ev_seg)
        HIP_TRY(h, hipEventCreateWithFlags(&h->ev_seg, hipEventDisableTiming));
    else
        HIP_TRY(h, hipEventSynchronize(h->ev_seg));
    if (n_seg > h->seg_host_n) {
        if (h->seg_host)
            HIP_TRY(h, hipHostFree(h->seg_host));
        h->seg_host = nullptr;
        h->seg_host_n = 0;
        HIP_TRY(h, hipHostMalloc((void **)&h->seg_host, (size_t)(2 * n_seg + 1) * sizeof(long long), hipHostMallocDefault));
        h->seg_host_n = n_seg;
    }
    memcpy(h->seg_host, seg_first, (size_t)(n_seg + 1) * sizeof(int64_t));
    memcpy(h->seg_host + n_seg + 1, limit_bytes, (size_t)n_seg * sizeof(int64_t));
    HIP_TRY(h, hipMemcpyAsync(h->ws_seg, h->seg_host, (size_t)(2 * n_seg + 1) * sizeof(long long), hipMemcpyHostToDevice, st));
    HIP_TRY(h, hipEventRecord(h->ev_seg, st));
    return PACX_OK;
}

/* The six solves, checked and launched in one place.  kind: SOLVE_RATE on a rate curve (curve, a, b = worst, bits,
   steps with rows of `row`; per_cf = budget) or SOLVE_BAND on a band curve (nmr, cap, cap_alloc; bit_alloc).
   segmented: n_seg segments from the host arrays seg_first and limit_bytes, uploaded.  Else the whole stream as one
   segment: seg_first is not given, limit_bytes points at the one limit, which reaches the device as an argument of
   the init kernel -- no staging buffer, no event, nothing the host waits for -- and the workspace grows to one state.
   peak (include/pacx.h, pacx_rate_solve_peak): a segmented solve whose limits are the peaks, with the stream's limit,
   the floors and the stream's result beside it and one more state, the stream's, behind the segments'. */
enum { SOLVE_RATE, SOLVE_BAND };
static int solve(pacx_handle *h, int kind, const char *what, int64_t n_cf, int32_t row, int32_t sub_stride,
                 const double *curve, const int32_t *a, const int32_t *b, bool segmented, int64_t n_seg,
                 const int64_t *seg_first, const int64_t *limit_bytes, double nmr_lo_db, double nmr_hi_db,
                 int32_t *per_cf, int32_t *n_bytes, uint8_t *capped, pacx_rate_result *result, void *stream,
                 const PacxSolveStream *peak = nullptr)
{
    if (!h)
        return PACX_E_ARG;
    if (int rc = scalar_only(h, what))
        return rc;
    if (n_cf < 0 || n_cf > 0x7fffffffLL / PACX_SUB)
        return fail(h, PACX_E_ARG, std::string(what) + ": bad channel-frame count");
    if (!result || (n_cf > 0 && (!curve || !a || !b || !per_cf || !n_bytes || !capped)) ||
        (peak && (!peak->floor || !peak->result)))
        return fail(h, PACX_E_ARG, std::string(what) + ": null pointer");
    if (kind == SOLVE_RATE && (sub_stride < 1 || row < (PACX_SUB - 1) * (long long)sub_stride + 1))
        return fail(h, PACX_E_ARG, std::string(what) + ": row must hold eight sub-blocks (row >= 7 sub_stride + 1)");
    int rc = PACX_OK, t_lo, t_hi;
    if (segmented)
        rc = check_segments(h, what, n_cf, n_seg, seg_first, limit_bytes);
    else if (*limit_bytes < 0)
        rc = fail(h, PACX_E_ARG, std::string(what) + ": negative limit");
    if (!rc && peak && peak->limit < 0)
        rc = fail(h, PACX_E_ARG, std::string(what) + ": negative limit");
    if (rc || (rc = solve_range(h, what, nmr_lo_db, nmr_hi_db, &t_lo, &t_hi)))
        return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    hipStream_t st = (hipStream_t)stream;
    if ((rc = segmented ? upload_segments(h, n_seg, seg_first, limit_bytes, peak ? 1 : 0, st) : grow(h, GROW_SOLVE, 1)))
        return rc;
    const PacxSolve v = {h->ws_solve, h->ws_seg, (int)n_seg, segmented ? nullptr : (const long long *)limit_bytes,
                         n_cf, t_lo, t_hi, result};
    if (peak && kind == SOLVE_RATE)
        pacx_launch_rate_solve_peak(v, *peak, row, sub_stride, curve, a, b, per_cf, n_bytes, capped, st);
    else if (peak)
        pacx_launch_band_solve_peak(h->T, v, *peak, curve, a, b, per_cf, n_bytes, capped, st);
    else if (kind == SOLVE_RATE)
        pacx_launch_rate_solve_segments(v, row, sub_stride, curve, a, b, per_cf, n_bytes, capped, st);
    else
        pacx_launch_band_solve_segments(h->T, v, curve, a, b, per_cf, n_bytes, capped, st);
    return post_launch(h, what);
}

extern "C" int pacx_rate_solve(pacx_handle *h, int64_t n_cf, int32_t row, int32_t sub_stride, const double *worst,
                               const int32_t *bits, const int32_t *steps, int64_t limit_bytes, double nmr_lo_db,
                               double nmr_hi_db, int32_t *budget, int32_t *n_bytes, uint8_t *capped,
                               pacx_rate_result *result, void *stream)
{
    return solve(h, SOLVE_RATE, "pacx_rate_solve", n_cf, row, sub_stride, worst, bits, steps, false, 1, nullptr,
                 &limit_bytes, nmr_lo_db, nmr_hi_db, budget, n_bytes, capped, result, stream);
}

extern "C" int pacx_rate_solve_segments(pacx_handle *h, int64_t n_cf, int32_t row, int32_t sub_stride,
                                        const double *worst, const int32_t *bits, const int32_t *steps, int64_t n_seg,
                                        const int64_t *seg_first, const int64_t *limit_bytes, double nmr_lo_db,
                                        double nmr_hi_db, int32_t *budget, int32_t *n_bytes, uint8_t *capped,
                                        pacx_rate_result *result, void *stream)
{
    return solve(h, SOLVE_RATE, "pacx_rate_solve_segments", n_cf, row, sub_stride, worst, bits, steps, true, n_seg,
                 seg_first, limit_bytes, nmr_lo_db, nmr_hi_db, budget, n_bytes, capped, result, stream);
}

extern "C" int pacx_rate_solve_peak(pacx_handle *h, int64_t n_cf, int32_t row, int32_t sub_stride, const double *worst,
                                    const int32_t *bits, const int32_t *steps, int64_t n_seg, const int64_t *seg_first,
                                    const int64_t *peak_bytes, int64_t limit_bytes, double nmr_lo_db, double nmr_hi_db,
                                    int32_t *budget, int32_t *n_bytes, uint8_t *capped, int32_t *floor,
                                    pacx_rate_result *result, pacx_rate_result *result_stream, void *stream)
{
    const PacxSolveStream peak = {limit_bytes, floor, result_stream};
    return solve(h, SOLVE_RATE, "pacx_rate_solve_peak", n_cf, row, sub_stride, worst, bits, steps, true, n_seg,
                 seg_first, peak_bytes, nmr_lo_db, nmr_hi_db, budget, n_bytes, capped, result, stream, &peak);
}

/* ---- bits handed to the bands one by one ---- */
extern "C" int pacx_band_pick(pacx_handle *h, int64_t n_cf, const double *nmr, const int32_t *cap, const int32_t *cap_alloc,
                              double target_nmr_db, int32_t *bit_alloc, int32_t *n_bytes, uint8_t *capped, void *stream)
{
    const char *what = "pacx_band_pick";
    if (!h)
        return PACX_E_ARG;
    if (int rc = scalar_only(h, what))
        return rc;
    if (n_cf < 0 || n_cf > 0x7fffffffLL / PACX_SUB)
        return fail(h, PACX_E_ARG, std::string(what) + ": bad channel-frame count");
    if (n_cf > 0 && (!nmr || !cap || !cap_alloc || !bit_alloc || !n_bytes || !capped))
        return fail(h, PACX_E_ARG, std::string(what) + ": null pointer");
    if (!std::isfinite(target_nmr_db))
        return fail(h, PACX_E_ARG, std::string(what) + ": target_nmr_db is not finite");
    HIP_TRY(h, hipSetDevice(h->device));
    pacx_launch_band_pick(h->T, n_cf, target_nmr_db, nmr, cap, cap_alloc, bit_alloc, n_bytes, capped, (hipStream_t)stream);
    return post_launch(h, what);
}

extern "C" int pacx_band_solve(pacx_handle *h, int64_t n_cf, const double *nmr, const int32_t *cap, const int32_t *cap_alloc,
                               int64_t limit_bytes, double nmr_lo_db, double nmr_hi_db, int32_t *bit_alloc,
                               int32_t *n_bytes, uint8_t *capped, pacx_rate_result *result, void *stream)
{
    return solve(h, SOLVE_BAND, "pacx_band_solve", n_cf, 0, 0, nmr, cap, cap_alloc, false, 1, nullptr, &limit_bytes,
                 nmr_lo_db, nmr_hi_db, bit_alloc, n_bytes, capped, result, stream);
}

extern "C" int pacx_band_solve_segments(pacx_handle *h, int64_t n_cf, const double *nmr, const int32_t *cap,
                                        const int32_t *cap_alloc, int64_t n_seg, const int64_t *seg_first,
                                        const int64_t *limit_bytes, double nmr_lo_db, double nmr_hi_db,
                                        int32_t *bit_alloc, int32_t *n_bytes, uint8_t *capped, pacx_rate_result *result,
                                        void *stream)
{
    return solve(h, SOLVE_BAND, "pacx_band_solve_segments", n_cf, 0, 0, nmr, cap, cap_alloc, true, n_seg, seg_first,
                 limit_bytes, nmr_lo_db, nmr_hi_db, bit_alloc, n_bytes, capped, result, stream);
}

extern "C" int pacx_band_solve_peak(pacx_handle *h, int64_t n_cf, const double *nmr, const int32_t *cap,
                                    const int32_t *cap_alloc, int64_t n_seg, const int64_t *seg_first,
                                    const int64_t *peak_bytes, int64_t limit_bytes, double nmr_lo_db, double nmr_hi_db,
                                    int32_t *bit_alloc, int32_t *n_bytes, uint8_t *capped, int32_t *floor,
                                    pacx_rate_result *result, pacx_rate_result *result_stream, void *stream)
{
    const PacxSolveStream peak = {limit_bytes, floor, result_stream};
    return solve(h, SOLVE_BAND, "pacx_band_solve_peak", n_cf, 0, 0, nmr, cap, cap_alloc, true, n_seg, seg_first,
                 peak_bytes, nmr_lo_db, nmr_hi_db, bit_alloc, n_bytes, capped, result, stream, &peak);
}

/* ---- a leaky bucket: its level at and through the hops (k_bucket.hip, k_bucket_pin.hip), the buffered solves and
   the pinned solves with a target per hop under it ---- */
static int check_bucket(pacx_handle *h, const char *what, int64_t n_hops, int32_t n_ch, const pacx_bucket *b)
{
    const int64_t most = 1LL << 30, size_most = 1LL << 40;
    if (!b)
        return fail(h, PACX_E_ARG, std::string(what) + ": null pointer");
    if (n_ch < 1 || n_hops < 0 || n_hops > most || n_hops * n_ch > most)
        return fail(h, PACX_E_ARG, std::string(what) + ": n_ch >= 1 and 0 <= n_hops n_ch <= 2^30");
    if (b->drain_q16 < 0 || b->size_bytes < 0 || b->size_bytes > size_most || b->start_q16 < 0 ||
        b->start_q16 > b->size_bytes << 16)
        return fail(h, PACX_E_ARG, std::string(what) + ": a bucket has drain_q16 >= 0, 0 <= size_bytes <= 2^40 and "
                                                       "0 <= start_q16 <= size_bytes << 16");
    return PACX_OK;
}

/* the two level scans, checked and launched in one place.  wants_through: the scan that also writes the level through
   every hop (k_bucket_pin.hip) */
static int bucket_scan(pacx_handle *h, const char *what, int64_t n_hops, int32_t n_ch, const int32_t *n_bytes,
                       const pacx_bucket *b, int64_t *level, bool wants_through, int64_t *through,
                       pacx_bucket_result *result, void *stream)
{
    if (!h)
        return PACX_E_ARG;
    if (int rc = check_bucket(h, what, n_hops, n_ch, b))
        return rc;
    if (!result || (n_hops > 0 && (!n_bytes || (wants_through && !through))))
        return fail(h, PACX_E_ARG, std::string(what) + ": null pointer");
    HIP_TRY(h, hipSetDevice(h->device));
    if (wants_through)
        pacx_launch_bucket_through(n_hops, n_ch, n_bytes, *b, level, through, result, (hipStream_t)stream);
    else
        pacx_launch_bucket_scan(n_hops, n_ch, n_bytes, *b, level, result, (hipStream_t)stream);
    return post_launch(h, what);
}

extern "C" int pacx_bucket_scan(pacx_handle *h, int64_t n_hops, int32_t n_ch, const int32_t *n_bytes, const pacx_bucket *b,
                                int64_t *level, pacx_bucket_result *result, void *stream)
{
    return bucket_scan(h, "pacx_bucket_scan", n_hops, n_ch, n_bytes, b, level, false, nullptr, result, stream);
}

extern "C" int pacx_bucket_through(pacx_handle *h, int64_t n_hops, int32_t n_ch, const int32_t *n_bytes,
                                   const pacx_bucket *b, int64_t *level, int64_t *through, pacx_bucket_result *result,
                                   void *stream)
{
    return bucket_scan(h, "pacx_bucket_through", n_hops, n_ch, n_bytes, b, level, true, through, result, stream);
}

/* what a pinned solve takes and gives beyond a buffered one (include/pacx_bucket_pin.h) */
struct PinArgs {
    int32_t pin_step_t, max_phases;
    int32_t *target_t, *phase_of;     /* [n_cf / n_ch] */
    pacx_pin_result *result;
};

/* The four solves under a bucket, checked and launched in one place: solve()'s rules for a whole-stream solve and
   check_bucket's.  Buffered: the picks are the one-segment picks of pacx_*_pick_segments at the state's target word.
   pin (k_bucket_pin.hip): the step and the phase count are checked too, the workspace holds F_h and a pin per hop,
   and the picks are those of pacx_*_pick_segments with a segment per hop at the solve's target_t. */
static int solve_bucket(pacx_handle *h, int kind, const char *what, int64_t n_cf, int32_t n_ch, int32_t row,
                        int32_t sub_stride, const double *curve, const int32_t *a, const int32_t *b, int64_t limit_bytes,
                        const pacx_bucket *bucket, double nmr_lo_db, double nmr_hi_db, int32_t *per_cf, int32_t *n_bytes,
                        uint8_t *capped, pacx_rate_result *result, pacx_bucket_result *bucket_result, void *stream,
                        const PinArgs *pin = nullptr)
{
    if (!h)
        return PACX_E_ARG;
    if (int rc = scalar_only(h, what))
        return rc;
    if (n_cf < 0 || n_cf > 0x7fffffffLL / PACX_SUB)
        return fail(h, PACX_E_ARG, std::string(what) + ": bad channel-frame count");
    if (n_ch < 1 || n_cf % n_ch != 0)
        return fail(h, PACX_E_ARG, std::string(what) + ": n_cf must be a multiple of n_ch >= 1");
    if (!result || !bucket_result || (pin && !pin->result) ||
        (n_cf > 0 && (!curve || !a || !b || !per_cf || !n_bytes || !capped || (pin && (!pin->target_t || !pin->phase_of)))))
        return fail(h, PACX_E_ARG, std::string(what) + ": null pointer");
    if (kind == SOLVE_RATE && (sub_stride < 1 || row < (PACX_SUB - 1) * (long long)sub_stride + 1))
        return fail(h, PACX_E_ARG, std::string(what) + ": row must hold eight sub-blocks (row >= 7 sub_stride + 1)");
    if (limit_bytes < 0)
        return fail(h, PACX_E_ARG, std::string(what) + ": negative limit");
    if (pin && pin->pin_step_t < 1)
        return fail(h, PACX_E_ARG, std::string(what) + ": pin_step_t must be at least 1 (grid units of 1/64 dB)");
    if (pin && (pin->max_phases < 1 || pin->max_phases > PACX_PIN_PHASES_MAX))
        return fail(h, PACX_E_ARG, std::string(what) + ": max_phases must lie in [1, " +
                                       std::to_string(PACX_PIN_PHASES_MAX) + "]");
    int rc, t_lo, t_hi;
    if ((rc = check_bucket(h, what, n_cf / n_ch, n_ch, bucket)) ||
        (rc = solve_range(h, what, nmr_lo_db, nmr_hi_db, &t_lo, &t_hi)))
        return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    hipStream_t st = (hipStream_t)stream;
    const int64_t n_hops = n_cf / n_ch;
    if ((rc = grow(h, GROW_SOLVE, pin && n_hops > 1 ? n_hops : 1)))
        return rc;
    /* a segment per hop at the pinned solve's targets, else one segment at the state's target word */
    auto pick = [&](long long seg_cf, const int32_t *target_t) {
        if (kind == SOLVE_RATE)
            pacx_launch_rate_pick_segments(n_cf, row, sub_stride, curve, a, b, seg_cf, 0, target_t, 0, per_cf, n_bytes,
                                           capped, st);
        else
            pacx_launch_band_pick_segments(h->T, n_cf, seg_cf, 0, target_t, curve, a, b, per_cf, n_bytes, capped, st);
    };
    if (pin) {
        const PacxPinSolve v = {h->ws_pin, n_cf, n_ch, t_lo, t_hi, pin->pin_step_t, pin->max_phases, limit_bytes, *bucket,
                                n_bytes, pin->target_t, pin->phase_of, result, bucket_result, pin->result};
        pacx_pin_drive(v, st, [&]() { pick(n_ch, pin->target_t); });
    } else {
        const PacxBucketSolve v = {h->ws_bucket, n_cf, n_ch, t_lo, t_hi, limit_bytes, *bucket, n_bytes, result,
                                   bucket_result};
        pacx_bucket_drive(v, st, [&](const int32_t *target_t) { pick(PACX_SEG_CF_MAX, target_t); });
    }
    return post_launch(h, what);
}

extern "C" int pacx_band_solve_bucket(pacx_handle *h, int64_t n_cf, int32_t n_ch, const double *nmr, const int32_t *cap,
                                      const int32_t *cap_alloc, int64_t limit_bytes, const pacx_bucket *b,
                                      double nmr_lo_db, double nmr_hi_db, int32_t *bit_alloc, int32_t *n_bytes,
                                      uint8_t *capped, pacx_rate_result *result, pacx_bucket_result *bucket_result,
                                      void *stream)
{
    return solve_bucket(h, SOLVE_BAND, "pacx_band_solve_bucket", n_cf, n_ch, 0, 0, nmr, cap, cap_alloc, limit_bytes, b,
                        nmr_lo_db, nmr_hi_db, bit_alloc, n_bytes, capped, result, bucket_result, stream);
}

extern "C" int pacx_rate_solve_bucket(pacx_handle *h, int64_t n_cf, int32_t n_ch, int32_t row, int32_t sub_stride,
                                      const double *worst, const int32_t *bits, const int32_t *steps,
                                      int64_t limit_bytes, const pacx_bucket *b, double nmr_lo_db, double nmr_hi_db,
                                      int32_t *budget, int32_t *n_bytes, uint8_t *capped, pacx_rate_result *result,
                                      pacx_bucket_result *bucket_result, void *stream)
{
    return solve_bucket(h, SOLVE_RATE, "pacx_rate_solve_bucket", n_cf, n_ch, row, sub_stride, worst, bits, steps,
                        limit_bytes, b, nmr_lo_db, nmr_hi_db, budget, n_bytes, capped, result, bucket_result, stream);
}

extern "C" int pacx_band_solve_bucket_pinned(pacx_handle *h, int64_t n_cf, int32_t n_ch, const double *nmr,
                                             const int32_t *cap, const int32_t *cap_alloc, int64_t limit_bytes,
                                             const pacx_bucket *b, double nmr_lo_db, double nmr_hi_db, int32_t pin_step_t,
                                             int32_t max_phases, int32_t *bit_alloc, int32_t *n_bytes, uint8_t *capped,
                                             int32_t *target_t, int32_t *phase_of, pacx_rate_result *result,
                                             pacx_bucket_result *bucket_result, pacx_pin_result *pin_result, void *stream)
{
    const PinArgs pin = {pin_step_t, max_phases, target_t, phase_of, pin_result};
    return solve_bucket(h, SOLVE_BAND, "pacx_band_solve_bucket_pinned", n_cf, n_ch, 0, 0, nmr, cap, cap_alloc, limit_bytes,
                        b, nmr_lo_db, nmr_hi_db, bit_alloc, n_bytes, capped, result, bucket_result, stream, &pin);
}

extern "C" int pacx_rate_solve_bucket_pinned(pacx_handle *h, int64_t n_cf, int32_t n_ch, int32_t row, int32_t sub_stride,
                                             const double *worst, const int32_t *bits, const int32_t *steps,
                                             int64_t limit_bytes, const pacx_bucket *b, double nmr_lo_db,
                                             double nmr_hi_db, int32_t pin_step_t, int32_t max_phases, int32_t *budget,
                                             int32_t *n_bytes, uint8_t *capped, int32_t *target_t, int32_t *phase_of,
                                             pacx_rate_result *result, pacx_bucket_result *bucket_result,
                                             pacx_pin_result *pin_result, void *stream)
{
    const PinArgs pin = {pin_step_t, max_phases, target_t, phase_of, pin_result};
    return solve_bucket(h, SOLVE_RATE, "pacx_rate_solve_bucket_pinned", n_cf, n_ch, row, sub_stride, worst, bits, steps,
                        limit_bytes, b, nmr_lo_db, nmr_hi_db, budget, n_bytes, capped, result, bucket_result, stream, &pin);
}

/* ---- the size at every target of the grid, and the solve on it ---- */
static int profile_range(pacx_handle *h, const char *what, double nmr_lo_db, double nmr_hi_db, int *t_lo, int *t_hi)
{
    if (int rc = solve_range(h, what, nmr_lo_db, nmr_hi_db, t_lo, t_hi))
        return rc;
    if ((long long)*t_hi - *t_lo + 1 > PACX_PROFILE_MAX)
        return fail(h, PACX_E_ARG, std::string(what) + ": a profile holds at most " + std::to_string(PACX_PROFILE_MAX) +
                                       " targets (a range of " +
                                       std::to_string((PACX_PROFILE_MAX - 1) / PACX_RATE_TARGET_GRID) + " dB)");
    return PACX_OK;
}

extern "C" int pacx_band_profile(pacx_handle *h, int64_t n_cf, const double *nmr, const int32_t *cap,
                                 const int32_t *cap_alloc, double nmr_lo_db, double nmr_hi_db, int64_t *profile,
                                 void *stream)
{
    const char *what = "pacx_band_profile";
    if (!h)
        return PACX_E_ARG;
    if (int rc = scalar_only(h, what))
        return rc;
    if (n_cf < 0 || n_cf > 0x7fffffffLL / PACX_SUB)
        return fail(h, PACX_E_ARG, std::string(what) + ": bad channel-frame count");
    if (!profile || (n_cf > 0 && (!nmr || !cap || !cap_alloc)))
        return fail(h, PACX_E_ARG, std::string(what) + ": null pointer");
    int t_lo, t_hi;
    if (int rc = profile_range(h, what, nmr_lo_db, nmr_hi_db, &t_lo, &t_hi))
        return rc;
    if (n_cf == 0)
        return PACX_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    pacx_launch_band_profile(h->T, n_cf, t_lo, t_hi, nmr, cap, cap_alloc, profile, (hipStream_t)stream);
    return post_launch(h, what);
}

extern "C" int pacx_profile_solve(pacx_handle *h, const int64_t *profile, int64_t limit_bytes, double nmr_lo_db,
                                  double nmr_hi_db, pacx_rate_result *result, void *stream)
{
    const char *what = "pacx_profile_solve";
    if (!h)
        return PACX_E_ARG;
    if (int rc = scalar_only(h, what))
        return rc;
    if (!profile || !result)
        return fail(h, PACX_E_ARG, std::string(what) + ": null pointer");
    if (limit_bytes < 0)
        return fail(h, PACX_E_ARG, std::string(what) + ": negative limit");
    int t_lo, t_hi;
    if (int rc = profile_range(h, what, nmr_lo_db, nmr_hi_db, &t_lo, &t_hi))
        return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    pacx_launch_profile_solve(profile, limit_bytes, t_lo, t_hi, result, (hipStream_t)stream);
    return post_launch(h, what);
}

/* ---- the same per uniform segment of a piece ---- */
/* what the two calls on a curve share: the handle's kind, the count, the segments given by value.  seg_cf is bounded
   so that first_off + cf stays far from the end of 64 bits in the kernels */
static int segments_by_value(pacx_handle *h, const char *what, int64_t n_cf, int64_t seg_cf, int64_t first_off)
{
    if (int rc = scalar_only(h, what))
        return rc;
    if (n_cf < 0 || n_cf > 0x7fffffffLL / PACX_SUB)
        return fail(h, PACX_E_ARG, std::string(what) + ": bad channel-frame count");
    if (seg_cf < 1 || seg_cf > PACX_SEG_CF_MAX)
        return fail(h, PACX_E_ARG, std::string(what) + ": seg_cf must lie in [1, 2^40]");
    if (first_off < 0 || first_off >= seg_cf)
        return fail(h, PACX_E_ARG, std::string(what) + ": first_off must lie in [0, seg_cf)");
    return PACX_OK;
}

extern "C" int pacx_band_profile_segments(pacx_handle *h, int64_t n_cf, const double *nmr, const int32_t *cap,
                                          const int32_t *cap_alloc, int64_t seg_cf, int64_t first_off, double nmr_lo_db,
                                          double nmr_hi_db, int64_t *profile, void *stream)
{
    const char *what = "pacx_band_profile_segments";
    if (!h)
        return PACX_E_ARG;
    int t_lo, t_hi;
    if (int rc = segments_by_value(h, what, n_cf, seg_cf, first_off))
        return rc;
    if (int rc = profile_range(h, what, nmr_lo_db, nmr_hi_db, &t_lo, &t_hi))
        return rc;
    if (!profile || (n_cf > 0 && (!nmr || !cap || !cap_alloc)))
        return fail(h, PACX_E_ARG, std::string(what) + ": null pointer");
    if (n_cf == 0)
        return PACX_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    pacx_launch_band_profile_segments(h->T, n_cf, seg_cf, first_off, t_lo, t_hi, nmr, cap, cap_alloc, profile,
                                      (hipStream_t)stream);
    return post_launch(h, what);
}

/* the two calls on rows alone */
static int rows_only(pacx_handle *h, const char *what, int64_t n_seg, const void *a, const void *b, const void *c,
                     double nmr_lo_db, double nmr_hi_db, int *t_lo, int *t_hi)
{
    if (int rc = scalar_only(h, what))
        return rc;
    if (n_seg < 1 || n_seg > 0x7fffffffLL / PACX_SUB)
        return fail(h, PACX_E_ARG, std::string(what) + ": bad segment count");
    if (!a || !b || !c)
        return fail(h, PACX_E_ARG, std::string(what) + ": null pointer");
    return profile_range(h, what, nmr_lo_db, nmr_hi_db, t_lo, t_hi);
}

extern "C" int pacx_profile_solve_segments(pacx_handle *h, int64_t n_seg, const int64_t *profile,
                                           const int64_t *limit_bytes, double nmr_lo_db, double nmr_hi_db,
                                           pacx_rate_result *result, int64_t *worst_above, void *stream)
{
    const char *what = "pacx_profile_solve_segments";
    if (!h)
        return PACX_E_ARG;
    int t_lo, t_hi;
    if (int rc = rows_only(h, what, n_seg, profile, limit_bytes, result, nmr_lo_db, nmr_hi_db, &t_lo, &t_hi))
        return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    pacx_launch_profile_solve_segments(n_seg, profile, limit_bytes, t_lo, t_hi, result, worst_above, (hipStream_t)stream);
    return post_launch(h, what);
}

extern "C" int pacx_profile_clamp_add(pacx_handle *h, int64_t n_seg, const int64_t *profile,
                                      const pacx_rate_result *result, double nmr_lo_db, double nmr_hi_db,
                                      int64_t *stream_profile, void *stream)
{
    const char *what = "pacx_profile_clamp_add";
    if (!h)
        return PACX_E_ARG;
    int t_lo, t_hi;
    if (int rc = rows_only(h, what, n_seg, profile, result, stream_profile, nmr_lo_db, nmr_hi_db, &t_lo, &t_hi))
        return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    pacx_launch_profile_clamp_add(n_seg, profile, result, t_lo, t_hi, stream_profile, (hipStream_t)stream);
    return post_launch(h, what);
}

extern "C" int pacx_band_pick_segments(pacx_handle *h, int64_t n_cf, const double *nmr, const int32_t *cap,
                                       const int32_t *cap_alloc, int64_t seg_cf, int64_t first_off,
                                       const int32_t *target_t, int32_t *bit_alloc, int32_t *n_bytes, uint8_t *capped,
                                       void *stream)
{
    const char *what = "pacx_band_pick_segments";
    if (!h)
        return PACX_E_ARG;
    if (int rc = segments_by_value(h, what, n_cf, seg_cf, first_off))
        return rc;
    if (n_cf > 0 && (!nmr || !cap || !cap_alloc || !target_t || !bit_alloc || !n_bytes || !capped))
        return fail(h, PACX_E_ARG, std::string(what) + ": null pointer");
    HIP_TRY(h, hipSetDevice(h->device));
    pacx_launch_band_pick_segments(h->T, n_cf, seg_cf, first_off, target_t, nmr, cap, cap_alloc, bit_alloc, n_bytes, capped,
                                   (hipStream_t)stream);
    return post_launch(h, what);
}

/* ---- the same on a rate curve: the profile, per stream and per uniform segment, and the pick at known targets ---- */
/* what the four calls share beyond segments_by_value: the row's layout (pacx_rate_solve's rule) */
static int rate_rows(pacx_handle *h, const char *what, int64_t n_cf, int64_t seg_cf, int64_t first_off, int32_t row,
                     int32_t sub_stride)
{
    if (int rc = segments_by_value(h, what, n_cf, seg_cf, first_off))
        return rc;
    if (sub_stride < 1 || row < (PACX_SUB - 1) * (long long)sub_stride + 1)
        return fail(h, PACX_E_ARG, std::string(what) + ": row must hold eight sub-blocks (row >= 7 sub_stride + 1)");
    return PACX_OK;
}

static int rate_profile(pacx_handle *h, const char *what, int64_t n_cf, int32_t row, int32_t sub_stride,
                        const double *worst, const int32_t *bits, const int32_t *steps, int64_t seg_cf,
                        int64_t first_off, double nmr_lo_db, double nmr_hi_db, int64_t *profile, void *stream)
{
    if (!h)
        return PACX_E_ARG;
    int t_lo, t_hi;
    if (int rc = rate_rows(h, what, n_cf, seg_cf, first_off, row, sub_stride))
        return rc;
    if (int rc = profile_range(h, what, nmr_lo_db, nmr_hi_db, &t_lo, &t_hi))
        return rc;
    if (!profile || (n_cf > 0 && (!worst || !bits || !steps)))
        return fail(h, PACX_E_ARG, std::string(what) + ": null pointer");
    if (n_cf == 0)
        return PACX_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    pacx_launch_rate_profile_segments(n_cf, row, sub_stride, worst, bits, steps, seg_cf, first_off, t_lo, t_hi, profile,
                                      (hipStream_t)stream);
    return post_launch(h, what);
}

extern "C" int pacx_rate_profile(pacx_handle *h, int64_t n_cf, int32_t row, int32_t sub_stride, const double *worst,
                                 const int32_t *bits, const int32_t *steps, double nmr_lo_db, double nmr_hi_db,
                                 int64_t *profile, void *stream)
{
    /* the whole stream is the one-segment case */
    return rate_profile(h, "pacx_rate_profile", n_cf, row, sub_stride, worst, bits, steps, PACX_SEG_CF_MAX, 0, nmr_lo_db,
                        nmr_hi_db, profile, stream);
}

extern "C" int pacx_rate_profile_segments(pacx_handle *h, int64_t n_cf, int32_t row, int32_t sub_stride,
                                          const double *worst, const int32_t *bits, const int32_t *steps, int64_t seg_cf,
                                          int64_t first_off, double nmr_lo_db, double nmr_hi_db, int64_t *profile,
                                          void *stream)
{
    return rate_profile(h, "pacx_rate_profile_segments", n_cf, row, sub_stride, worst, bits, steps, seg_cf, first_off,
                        nmr_lo_db, nmr_hi_db, profile, stream);
}

static int rate_pick(pacx_handle *h, const char *what, int64_t n_cf, int32_t row, int32_t sub_stride,
                     const double *worst, const int32_t *bits, const int32_t *steps, int64_t seg_cf, int64_t first_off,
                     const int32_t *target_t, bool by_segment, int t_all, int32_t *budget, int32_t *n_bytes,
                     uint8_t *capped, void *stream)
{
    if (int rc = rate_rows(h, what, n_cf, seg_cf, first_off, row, sub_stride))
        return rc;
    if (n_cf > 0 && (!worst || !bits || !steps || (by_segment && !target_t) || !budget || !n_bytes || !capped))
        return fail(h, PACX_E_ARG, std::string(what) + ": null pointer");
    HIP_TRY(h, hipSetDevice(h->device));
    pacx_launch_rate_pick_segments(n_cf, row, sub_stride, worst, bits, steps, seg_cf, first_off,
                                   by_segment ? target_t : nullptr, t_all, budget, n_bytes, capped, (hipStream_t)stream);
    return post_launch(h, what);
}

extern "C" int pacx_rate_pick(pacx_handle *h, int64_t n_cf, int32_t row, int32_t sub_stride, const double *worst,
                              const int32_t *bits, const int32_t *steps, double target_nmr_db, int32_t *budget,
                              int32_t *n_bytes, uint8_t *capped, void *stream)
{
    const char *what = "pacx_rate_pick";
    if (!h)
        return PACX_E_ARG;
    if (int rc = scalar_only(h, what))
        return rc;
    int t, t_same;                                 /* the target on the grid: solve_range's rules for one bound */
    if (int rc = solve_range(h, what, target_nmr_db, target_nmr_db, &t, &t_same))
        return rc;
    return rate_pick(h, what, n_cf, row, sub_stride, worst, bits, steps, PACX_SEG_CF_MAX, 0, nullptr, false, t, budget,
                     n_bytes, capped, stream);
}

extern "C" int pacx_rate_pick_segments(pacx_handle *h, int64_t n_cf, int32_t row, int32_t sub_stride,
                                       const double *worst, const int32_t *bits, const int32_t *steps, int64_t seg_cf,
                                       int64_t first_off, const int32_t *target_t, int32_t *budget, int32_t *n_bytes,
                                       uint8_t *capped, void *stream)
{
    if (!h)
        return PACX_E_ARG;
    return rate_pick(h, "pacx_rate_pick_segments", n_cf, row, sub_stride, worst, bits, steps, seg_cf, first_off, target_t,
                     true, 0, budget, n_bytes, capped, stream);
}

/* ---- a curve kept as grid indices, and the picks on it (k_kept.hip) ---- */
static bool aligned16(const void *p) { return ((uintptr_t)p & 15u) == 0; }

/* a target given by value: on the grid (solve_range's rules for one bound) and inside the range */
static int kept_target(pacx_handle *h, const char *what, double target_nmr_db, int t_lo, int t_hi, int *t)
{
    int t_same;
    if (int rc = solve_range(h, what, target_nmr_db, target_nmr_db, t, &t_same))
        return rc;
    if (*t < t_lo || *t > t_hi)
        return fail(h, PACX_E_ARG, std::string(what) + ": target_nmr_db lies outside [nmr_lo_db, nmr_hi_db]");
    return PACX_OK;
}

extern "C" int pacx_band_thresholds(pacx_handle *h, int64_t n_cf, const double *nmr, const int32_t *cap,
                                    const int32_t *cap_alloc, double nmr_lo_db, double nmr_hi_db, uint16_t *e,
                                    int32_t *kept_cap, uint8_t *kept_cap_alloc, void *stream)
{
    const char *what = "pacx_band_thresholds";
    if (!h)
        return PACX_E_ARG;
    int t_lo, t_hi;
    if (int rc = segments_by_value(h, what, n_cf, PACX_SEG_CF_MAX, 0))
        return rc;
    if (int rc = profile_range(h, what, nmr_lo_db, nmr_hi_db, &t_lo, &t_hi))
        return rc;
    if (n_cf > 0 && (!nmr || !cap || !cap_alloc || !e || !kept_cap || !kept_cap_alloc))
        return fail(h, PACX_E_ARG, std::string(what) + ": null pointer");
    if (!aligned16(nmr) || !aligned16(e))
        return fail(h, PACX_E_ARG, std::string(what) + ": nmr and e must be 16-byte aligned");
    if (n_cf == 0)
        return PACX_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    pacx_launch_band_thresholds(h->T, n_cf, t_lo, t_hi, nmr, cap, cap_alloc, e, kept_cap, kept_cap_alloc,
                                (hipStream_t)stream);
    return post_launch(h, what);
}

static int band_pick_kept(pacx_handle *h, const char *what, int64_t n_cf, const uint16_t *e, const int32_t *cap,
                          const uint8_t *cap_alloc, int64_t seg_cf, int64_t first_off, double nmr_lo_db, double nmr_hi_db,
                          const int32_t *target_t, const double *target_nmr_db, int32_t *bit_alloc, int32_t *n_bytes,
                          uint8_t *capped, void *stream)
{
    int t_lo, t_hi, t_all = 0;
    if (int rc = segments_by_value(h, what, n_cf, seg_cf, first_off))
        return rc;
    if (int rc = profile_range(h, what, nmr_lo_db, nmr_hi_db, &t_lo, &t_hi))
        return rc;
    if (target_nmr_db)
        if (int rc = kept_target(h, what, *target_nmr_db, t_lo, t_hi, &t_all))
            return rc;
    if (n_cf > 0 && (!e || !cap || !cap_alloc || (!target_nmr_db && !target_t) || !bit_alloc || !n_bytes || !capped))
        return fail(h, PACX_E_ARG, std::string(what) + ": null pointer");
    if (!aligned16(e))
        return fail(h, PACX_E_ARG, std::string(what) + ": e must be 16-byte aligned");
    if (n_cf == 0)
        return PACX_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    pacx_launch_band_pick_thresholds(h->T, n_cf, seg_cf, first_off, target_nmr_db ? nullptr : target_t, t_all, t_lo, t_hi,
                                     e, cap, cap_alloc, bit_alloc, n_bytes, capped, (hipStream_t)stream);
    return post_launch(h, what);
}

extern "C" int pacx_band_pick_thresholds(pacx_handle *h, int64_t n_cf, const uint16_t *e, const int32_t *cap,
                                         const uint8_t *cap_alloc, double nmr_lo_db, double nmr_hi_db,
                                         double target_nmr_db, int32_t *bit_alloc, int32_t *n_bytes, uint8_t *capped,
                                         void *stream)
{
    if (!h)
        return PACX_E_ARG;
    return band_pick_kept(h, "pacx_band_pick_thresholds", n_cf, e, cap, cap_alloc, PACX_SEG_CF_MAX, 0, nmr_lo_db,
                          nmr_hi_db, nullptr, &target_nmr_db, bit_alloc, n_bytes, capped, stream);
}

extern "C" int pacx_band_pick_thresholds_segments(pacx_handle *h, int64_t n_cf, const uint16_t *e, const int32_t *cap,
                                                  const uint8_t *cap_alloc, int64_t seg_cf, int64_t first_off,
                                                  double nmr_lo_db, double nmr_hi_db, const int32_t *target_t,
                                                  int32_t *bit_alloc, int32_t *n_bytes, uint8_t *capped, void *stream)
{
    if (!h)
        return PACX_E_ARG;
    return band_pick_kept(h, "pacx_band_pick_thresholds_segments", n_cf, e, cap, cap_alloc, seg_cf, first_off, nmr_lo_db,
                          nmr_hi_db, target_t, nullptr, bit_alloc, n_bytes, capped, stream);
}

extern "C" int pacx_rate_thresholds(pacx_handle *h, int64_t n_cf, int32_t row, int32_t sub_stride, const double *worst,
                                    const int32_t *bits, const int32_t *steps, double nmr_lo_db, double nmr_hi_db,
                                    uint16_t *e, int32_t *kept_bits, int32_t *kept_steps, void *stream)
{
    const char *what = "pacx_rate_thresholds";
    if (!h)
        return PACX_E_ARG;
    int t_lo, t_hi;
    if (int rc = rate_rows(h, what, n_cf, PACX_SEG_CF_MAX, 0, row, sub_stride))
        return rc;
    if (int rc = profile_range(h, what, nmr_lo_db, nmr_hi_db, &t_lo, &t_hi))
        return rc;
    if (n_cf > 0 && (!worst || !bits || !steps || !e || !kept_bits || !kept_steps))
        return fail(h, PACX_E_ARG, std::string(what) + ": null pointer");
    if (n_cf == 0)
        return PACX_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    pacx_launch_rate_thresholds(n_cf, row, sub_stride, t_lo, t_hi, worst, bits, steps, e, kept_bits, kept_steps,
                                (hipStream_t)stream);
    return post_launch(h, what);
}

static int rate_pick_kept(pacx_handle *h, const char *what, int64_t n_cf, int32_t row, int32_t sub_stride,
                          const uint16_t *e, const int32_t *bits, const int32_t *steps, int64_t seg_cf, int64_t first_off,
                          double nmr_lo_db, double nmr_hi_db, const int32_t *target_t, const double *target_nmr_db,
                          int32_t *budget, int32_t *n_bytes, uint8_t *capped, void *stream)
{
    int t_lo, t_hi, t_all = 0;
    if (int rc = rate_rows(h, what, n_cf, seg_cf, first_off, row, sub_stride))
        return rc;
    if (int rc = profile_range(h, what, nmr_lo_db, nmr_hi_db, &t_lo, &t_hi))
        return rc;
    if (target_nmr_db)
        if (int rc = kept_target(h, what, *target_nmr_db, t_lo, t_hi, &t_all))
            return rc;
    if (n_cf > 0 && (!e || !bits || !steps || (!target_nmr_db && !target_t) || !budget || !n_bytes || !capped))
        return fail(h, PACX_E_ARG, std::string(what) + ": null pointer");
    if (n_cf == 0)
        return PACX_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    pacx_launch_rate_pick_thresholds(n_cf, row, sub_stride, seg_cf, first_off, target_nmr_db ? nullptr : target_t, t_all,
                                     t_lo, t_hi, e, bits, steps, budget, n_bytes, capped, (hipStream_t)stream);
    return post_launch(h, what);
}

extern "C" int pacx_rate_pick_thresholds(pacx_handle *h, int64_t n_cf, int32_t row, int32_t sub_stride, const uint16_t *e,
                                         const int32_t *bits, const int32_t *steps, double nmr_lo_db, double nmr_hi_db,
                                         double target_nmr_db, int32_t *budget, int32_t *n_bytes, uint8_t *capped,
                                         void *stream)
{
    if (!h)
        return PACX_E_ARG;
    return rate_pick_kept(h, "pacx_rate_pick_thresholds", n_cf, row, sub_stride, e, bits, steps, PACX_SEG_CF_MAX, 0,
                          nmr_lo_db, nmr_hi_db, nullptr, &target_nmr_db, budget, n_bytes, capped, stream);
}

extern "C" int pacx_rate_pick_thresholds_segments(pacx_handle *h, int64_t n_cf, int32_t row, int32_t sub_stride,
                                                  const uint16_t *e, const int32_t *bits, const int32_t *steps,
                                                  int64_t seg_cf, int64_t first_off, double nmr_lo_db, double nmr_hi_db,
                                                  const int32_t *target_t, int32_t *budget, int32_t *n_bytes,
                                                  uint8_t *capped, void *stream)
{
    if (!h)
        return PACX_E_ARG;
    return rate_pick_kept(h, "pacx_rate_pick_thresholds_segments", n_cf, row, sub_stride, e, bits, steps, seg_cf,
                          first_off, nmr_lo_db, nmr_hi_db, target_t, nullptr, budget, n_bytes, capped, stream);
}

/* ---- the buffered solve for a stream in chunks, on kept curves (k_bucket_kept.hip, include/pacx_bucket_kept.h) ---- */
static int tree_targets(pacx_handle *h, const char *what, int32_t n_targets)
{
    if (n_targets < 1 || n_targets > PACX_BUCKET_TREE_TARGETS)
        return fail(h, PACX_E_ARG, std::string(what) + ": n_targets must lie in [1, " +
                                       std::to_string(PACX_BUCKET_TREE_TARGETS) + "]");
    return PACX_OK;
}

extern "C" int pacx_band_bytes_thresholds(pacx_handle *h, int64_t n_cf, const uint16_t *e, const int32_t *cap,
                                          const uint8_t *cap_alloc, double nmr_lo_db, double nmr_hi_db, int32_t n_targets,
                                          const int32_t *target_t, int32_t *n_bytes_t, void *stream)
{
    const char *what = "pacx_band_bytes_thresholds";
    if (!h)
        return PACX_E_ARG;
    int t_lo, t_hi;
    if (int rc = segments_by_value(h, what, n_cf, PACX_SEG_CF_MAX, 0))
        return rc;
    if (int rc = profile_range(h, what, nmr_lo_db, nmr_hi_db, &t_lo, &t_hi))
        return rc;
    if (int rc = tree_targets(h, what, n_targets))
        return rc;
    if (n_cf > 0 && (!e || !cap || !cap_alloc || !target_t || !n_bytes_t))
        return fail(h, PACX_E_ARG, std::string(what) + ": null pointer");
    if (!aligned16(e))
        return fail(h, PACX_E_ARG, std::string(what) + ": e must be 16-byte aligned");
    if (n_cf == 0)
        return PACX_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    pacx_launch_band_bytes_thresholds(h->T, n_cf, n_targets, target_t, t_lo, t_hi, e, cap, cap_alloc, n_bytes_t,
                                      (hipStream_t)stream);
    return post_launch(h, what);
}

extern "C" int pacx_rate_bytes_thresholds(pacx_handle *h, int64_t n_cf, int32_t row, int32_t sub_stride, const uint16_t *e,
                                          const int32_t *bits, const int32_t *steps, double nmr_lo_db, double nmr_hi_db,
                                          int32_t n_targets, const int32_t *target_t, int32_t *n_bytes_t, void *stream)
{
    const char *what = "pacx_rate_bytes_thresholds";
    if (!h)
        return PACX_E_ARG;
    int t_lo, t_hi;
    if (int rc = rate_rows(h, what, n_cf, PACX_SEG_CF_MAX, 0, row, sub_stride))
        return rc;
    if (int rc = profile_range(h, what, nmr_lo_db, nmr_hi_db, &t_lo, &t_hi))
        return rc;
    if (int rc = tree_targets(h, what, n_targets))
        return rc;
    if (n_cf > 0 && (!e || !bits || !steps || !target_t || !n_bytes_t))
        return fail(h, PACX_E_ARG, std::string(what) + ": null pointer");
    if (n_cf == 0)
        return PACX_OK;
    HIP_TRY(h, hipSetDevice(h->device));
    pacx_launch_rate_bytes_thresholds(n_cf, row, sub_stride, n_targets, target_t, t_lo, t_hi, e, bits, steps, n_bytes_t,
                                      (hipStream_t)stream);
    return post_launch(h, what);
}

extern "C" int pacx_bucket_scan_targets(pacx_handle *h, int64_t n_hops, int32_t n_ch, int32_t n_targets,
                                        const int32_t *n_bytes_t, int64_t row_stride, int64_t drain_q16,
                                        int64_t size_bytes, int64_t hop_off, pacx_bucket_result *acc, void *stream)
{
    const char *what = "pacx_bucket_scan_targets";
    if (!h)
        return PACX_E_ARG;
    const pacx_bucket b = {drain_q16, size_bytes, 0};                 /* every target starts where its acc ended */
    if (int rc = check_bucket(h, what, n_hops, n_ch, &b))
        return rc;
    if (int rc = tree_targets(h, what, n_targets))
        return rc;
    if (hop_off < 0 || hop_off > (1LL << 30) - n_hops)
        return fail(h, PACX_E_ARG, std::string(what) + ": hop_off >= 0 and hop_off + n_hops <= 2^30");
    if (n_hops > 0 && row_stride < n_hops * n_ch)
        return fail(h, PACX_E_ARG, std::string(what) + ": row_stride must hold a row (row_stride >= n_hops n_ch)");
    if (!acc || (n_hops > 0 && !n_bytes_t))
        return fail(h, PACX_E_ARG, std::string(what) + ": null pointer");
    if (n_hops == 0)
        return PACX_OK;                            /* the piece of no hop leaves every acc as it is */
    HIP_TRY(h, hipSetDevice(h->device));
    pacx_launch_bucket_scan_targets(n_hops, n_ch, n_targets, n_bytes_t, row_stride, drain_q16, size_bytes, hop_off, acc,
                                    (hipStream_t)stream);
    return post_launch(h, what);
}

/* what the two tree calls refuse alike */
static int tree_args(pacx_handle *h, const char *what, const pacx_bucket *b, int32_t levels, const void *state,
                     const int32_t *target_t, const pacx_bucket_result *acc)
{
    if (!b || !state || !target_t || !acc)
        return fail(h, PACX_E_ARG, std::string(what) + ": null pointer");
    if (levels < 1 || levels > PACX_BUCKET_TREE_LEVELS_MAX)
        return fail(h, PACX_E_ARG, std::string(what) + ": levels must lie in [1, " +
                                       std::to_string(PACX_BUCKET_TREE_LEVELS_MAX) + "]");
    return check_bucket(h, what, 0, 1, b);
}

extern "C" int pacx_bucket_tree_begin(pacx_handle *h, const pacx_bucket *b, double nmr_lo_db, double nmr_hi_db,
                                      int32_t levels, void *state, int32_t *target_t, pacx_bucket_result *acc,
                                      void *stream)
{
    const char *what = "pacx_bucket_tree_begin";
    if (!h)
        return PACX_E_ARG;
    int t_lo, t_hi;
    if (int rc = tree_args(h, what, b, levels, state, target_t, acc))
        return rc;
    if (int rc = solve_range(h, what, nmr_lo_db, nmr_hi_db, &t_lo, &t_hi))
        return rc;
    HIP_TRY(h, hipSetDevice(h->device));
    pacx_launch_bucket_tree_begin(state, t_lo, t_hi, levels, b->start_q16, target_t, acc, (hipStream_t)stream);
    return post_launch(h, what);
}

extern "C" int pacx_bucket_tree_step(pacx_handle *h, int64_t limit_bytes, const pacx_bucket *b, int32_t levels,
                                     void *state, int32_t *target_t, pacx_bucket_result *acc, pacx_rate_result *result,
                                     pacx_bucket_result *bucket_result, void *stream)
{
    const char *what = "pacx_bucket_tree_step";
    if (!h)
        return PACX_E_ARG;
    if (int rc = tree_args(h, what, b, levels, state, target_t, acc))
        return rc;
    if (!result || !bucket_result)
        return fail(h, PACX_E_ARG, std::string(what) + ": null pointer");
    if (limit_bytes < 0)
        return fail(h, PACX_E_ARG, std::string(what) + ": negative limit");
    HIP_TRY(h, hipSetDevice(h->device));
    pacx_launch_bucket_tree_step(state, limit_bytes, b->size_bytes, b->start_q16, levels, target_t, acc, result,
                                 bucket_result, (hipStream_t)stream);
    return post_launch(h, what);
}

extern "C" int pacx_nmr_summary(pacx_handle *h, int64_t n_cf, int n_channels, const uint8_t *frame_flags,
                                const double *nmr_db, uint64_t *summary, void *stream)
{
    if (!h)
        return PACX_E_ARG;
    if (n_cf == 0)
        return PACX_OK;
    if (n_cf < 0 || n_cf > 0x7fffffffLL / PACX_SUB || n_channels < 1 || !nmr_db || !summary)
        return fail(h, PACX_E_ARG, "pacx_nmr_summary: bad argument");
    HIP_TRY(h, hipSetDevice(h->device));
    pacx_launch_nmr_summary(h->T, frame_flags, n_channels, n_cf, nmr_db, (unsigned long long *)summary,
                            (hipStream_t)stream);
    return post_launch(h, "pacx_nmr_summary");
}
