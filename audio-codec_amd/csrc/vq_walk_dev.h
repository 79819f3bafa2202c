/*
 * vq_walk_dev.h -- the passes of the gain-shape LEVEL walk and its stream layout, declared once.
 *
 * k_vq.hip walks one split tree three ways.  vq_shape goes depth first and writes as it goes; vq_shape_bfs (one band,
 * one wave) and the level loop of k_vq_frame (all bands of a unit, four waves) go level by level, keep every node's
 * field in a VqStore and lay the stream out at the end.  What these two do to a node stands here: the folds
 * (vq_fold_wide is vq_shape's too), the leaf passes, a split's scalar stage, the birth of its children, the layout and
 * the field writer.  What differs stays with the walkers: which nodes form a pass and which wave takes it (sl / ll
 * against ord / cls, the dealing and role rotation of k_vq_frame), where a level's vectors lie, how node numbers are
 * handed out, the measuring stamps around the calls.
 *
 * Included by k_vq.hip behind what it calls (VqView, ldc, vq_atan, vq_log2_tan, the wave sums and scans, vq_leaf_idx,
 * vq_leaf_group).  The scalar rule is vq_exact.h's, which takes no pointers: a split's two table values come in
 * through the walker's own fetch (global loads in vq_shape_bfs, the LDS copies in k_vq_frame).
 */
#pragma once

/* who strides a store's nodes in the layout passes, and what separates two levels: one wave or the workgroup */
template <int THREADS> struct VqTeam {
    static constexpr int size = THREADS;
    static __device__ __forceinline__ void sync() { THREADS == 64 ? wave_lds_fence() : __syncthreads(); }
};

/* ---- the node store --------------------------------------------------------- */
/* NC nodes, numbered in Idx; the two children of a split are born side by side, so kid[] holds the first and has[] says
   which exist (1: mid, 2: side).  BANDS: nodes of several bands' trees, band[] says whose. */
template <int NC, typename Idx, bool BANDS> struct VqStore {
    static constexpr int node_bytes = NC * (8 + 5 * 2 + (int)sizeof(Idx) + (BANDS ? 4 : 3));
    static constexpr bool bands = BANDS;
    typedef Idx index_t;
    unsigned long long *val;           /* [NC] field value (a split's |side|/|mid| while its level is open) */
    unsigned short *nn, *bb, *off, *tot, *pos;   /* [NC] length, bits, vector offset, subtree bits, stream bit */
    Idx *kid;                          /* [NC] first child */
    unsigned char *kind, *wid, *band, *has;      /* [NC] 0 split / 1 leaf / 3 leaf without a field; field width; band; children */
    Idx *lvl;                          /* [VQ_DEPTH + 2] first node of every depth (the walker places it) */
    /* returns the first byte behind the nodes: the walker's level lists follow */
    __device__ __forceinline__ unsigned char *bind_nodes(unsigned char *p)
    {
        val = (unsigned long long *)p;
        nn = (unsigned short *)(p + NC * 8);
        bb = nn + NC;
        off = bb + NC;
        tot = off + NC;
        pos = tot + NC;
        kid = (Idx *)(pos + NC);
        kind = (unsigned char *)(kid + NC);
        wid = kind + NC;
        band = wid + NC;
        has = BANDS ? band + NC : band;       /* without BANDS band[] IS has[]: touch it behind S::bands only */
        return has + NC;
    }
};

/* a field of up to 64 bits, by ONE lane (fields of different lanes may share words) */
__device__ __forceinline__ void vq_put_field(unsigned *words, int pos, unsigned long long val, int width)
{
    const int w = pos >> 5, t = (pos & 31) + width;
    if (t <= 32) {
        atomicOr(&words[w], (unsigned)val << (32 - t));
    } else if (t <= 64) {
        const unsigned long long v = val << (64 - t);
        atomicOr(&words[w], (unsigned)(v >> 32));
        atomicOr(&words[w + 1], (unsigned)v);
    } else {
        const int r = t - 64;
        const unsigned long long v = val >> r;
        atomicOr(&words[w], (unsigned)(v >> 32));
        atomicOr(&words[w + 1], (unsigned)v);
        atomicOr(&words[w + 2], (unsigned)val << (32 - r));
    }
}

/* ---- folds ------------------------------------------------------------------ */
__device__ __forceinline__ void vq_mid_side(double left, double right, double &m, double &s)
{
    m = (left + right) / 2.0;
    s = (left - right) / 2.0;
}

/* what a split keeps of its fold until the scalar stage: |side| / |mid| as a word, -1.0 for a mid half of norm zero */
__device__ __forceinline__ unsigned long long vq_ratio_word(double m_l2, double s_l2)
{
    return (unsigned long long)__double_as_longlong(m_l2 == 0.0 ? -1.0 : s_l2 / m_l2);
}

/* src[0 .. cut + half) -> unit mid and side halves mv, sv (half = ceil(n/2) each, cut = n/2), lanes strided over the half; the ratio word in every lane */
__device__ __forceinline__ unsigned long long vq_fold_wide(const double *src, int cut, int half, double *mv, double *sv,
                                                           int lane)
{
    double mm = 0.0, ss = 0.0;
    for (int i = lane; i < half; i += 64) {
        const double left = (i < cut) ? src[i] : 0.0;
        const double right = src[cut + i];
        double mid, sd;
        vq_mid_side(left, right, mid, sd);
        mv[i] = mid;
        sv[i] = sd;
        mm = fma(mid, mid, mm);
        ss = fma(sd, sd, ss);
    }
    const double m_l2 = sqrt(wave_sum_f64(mm));
    const double s_l2 = sqrt(wave_sum_f64(ss));
    for (int i = lane; i < half; i += 64) {
        if (m_l2 != 0.0)
            mv[i] = mv[i] / m_l2;
        if (s_l2 != 0.0)
            sv[i] = sv[i] / s_l2;
    }
    return vq_ratio_word(m_l2, s_l2);
}

/* one node per aligned block of P = 1 << lp lanes (half <= P; i: this lane's place in its block): the block folds cur + off[node] into nxt + tot[node]; the
   xor butterfly over a block adds in the order of the 64-lane one.  head: this lane stores the returned ratio word */
template <class S>
__device__ __forceinline__ unsigned long long vq_fold_packed(const S &N, const double *cur, double *nxt, int lp, bool valid,
                                                             int node, int i, bool &head)
{
    const int P = 1 << lp;
    const int n = valid ? N.nn[node] : 0;
    const int cut = n / 2, half = n - cut;
    const double *src = cur + (valid ? N.off[node] : 0);
    const bool mine = i < half;
    const double left = (mine && i < cut) ? src[i] : 0.0;
    const double right = mine ? src[cut + i] : 0.0;
    double m, s;
    vq_mid_side(left, right, m, s);
    double mid = mine ? m : 0.0;
    double sd = mine ? s : 0.0;
    double mm = fma(mid, mid, 0.0), ss = fma(sd, sd, 0.0);
    for (int off = P >> 1; off > 0; off >>= 1) {
        mm = mm + __shfl_xor(mm, off, 64);
        ss = ss + __shfl_xor(ss, off, 64);
    }
    const double m_l2 = sqrt(mm), s_l2 = sqrt(ss);
    if (m_l2 != 0.0)
        mid = mid / m_l2;
    if (s_l2 != 0.0)
        sd = sd / s_l2;
    if (mine) {
        double *mv = nxt + N.tot[node];
        mv[i] = mid;
        mv[half + i] = sd;
    }
    head = valid && i == 0;
    return vq_ratio_word(m_l2, s_l2);
}

/* ---- leaves ----------------------------------------------------------------- */
/* 64 >> lw leaves of up to 1 << lw components (lw = 4 or 5), one per group of lanes; `node` is this group's (valid: it has
   one), l this lane's place in the group.  Pulse count and index width are looked up here, beside the scalar stage, not in it.  GUARD: the margins of
   PACX_ST_GUARD are taken (by a copy of the leaf code of its own) */
template <bool ROWS64, bool GUARD, class S>
__device__ __forceinline__ void vq_leaf_pass(const VqView &V, const S &N, const double *cur, int lw, bool valid, int node,
                                             int l, bool &undefined, bool &guarded)
{
    const int n = valid ? N.nn[node] : 0;
    int bits = valid ? N.bb[node] : 0;
    bits = bits > 32 ? 32 : bits;
    const int K = valid ? V.tab.k_of[n * 33 + bits] : 0;
    const int width = valid ? V.tab.w_of[n * 33 + bits] : 0;
    const double x = (valid && l < n) ? cur[N.off[node] + l] : 0.0;
    bool ok = false, near = false;
    unsigned long long term;
    if (lw == 4)
        term = vq_leaf_group<16, ROWS64>(V, x, n, K < 0 ? 0 : K, l, ok, GUARD, &near);
    else
        term = vq_leaf_group<32, ROWS64>(V, x, n, K < 0 ? 0 : K, l, ok, GUARD, &near);
    if (GUARD)
        guarded = guarded || (valid && near);
    if (valid && l == 0) {
        if (K < 0) {                               /* a 1-dimensional leaf: the reference never returns */
            N.kind[node] = 3;
            N.wid[node] = 0;
            N.val[node] = 0ull;
        } else {
            N.val[node] = ok ? term : 0ull;
            N.wid[node] = (unsigned char)width;
        }
    }
    if (valid && (K < 0 || !ok))
        undefined = true;
}

/* a leaf of more than 32 components on the whole wave; t1: 2 n doubles of scratch */
template <bool ROWS64, class S>
__device__ __forceinline__ void vq_leaf_whole(const VqView &V, const S &N, const double *cur, double *t1, int node, int lane,
                                              bool &undefined)
{
    const int n = N.nn[node];
    int bits = N.bb[node];
    bits = bits > 32 ? 32 : bits;
    const int K = ldc(&V.tab.k_of[n * 33 + bits]);
    const int width = ldc(&V.tab.w_of[n * 33 + bits]);
    bool ok = true;
    const unsigned long long idx = vq_leaf_idx<ROWS64>(V, cur + N.off[node], n, K, t1, t1 + n, lane, ok);
    if (!ok)
        undefined = true;
    if (lane == 0) {
        N.val[node] = ok ? idx : 0ull;
        N.wid[node] = (unsigned char)width;
    }
}

/* ---- a split's scalar stage, one split per lane ----------------------------- */
struct VqSplit {
    unsigned long long code;           /* the angle's field ... */
    int w_theta;                       /* ... and its width */
    int a_mid, a_side;                 /* bits of the two halves */
    int c_mid, c_side;                 /* 1: that child exists */
    int rel, born;                     /* children of the lanes below; of the whole wave */
};

/* has: this lane holds a split of `bits` bits whose fold left the ratio word q; half = ceil(n / 2) (1 in idle lanes).
   half_log2(half) and log2_tan(slot) fetch the two table values the walker's way; stamp(k) is the walker's measuring
   hook (slots 26..28 of g_vq_dbg), nothing by default.  Where no angle of the wave has more than 31 bits (all but freak
   allocations) code and value take vq_exact.h's 32-bit form, equal to the 64-bit one (tests/test_host_exact.py).
   GUARD: a split angle within rounding distance of a boundary of its quantiser raises `guarded` */
template <bool GUARD, bool ANGLE32, class HalfLog2, class Log2Tan, class Stamp>
__device__ __forceinline__ VqSplit vq_split_stage(bool has, int bits, int half, double q, int lane, HalfLog2 half_log2,
                                                  Log2Tan log2_tan, Stamp stamp, bool &undefined, bool &guarded)
{
    VqSplit s;
    const double theta = (q < 0.0) ? 0.0 : vq_atan(q);
    stamp(26);
    const double hl = half_log2(half);
    const int a_theta = vq_first_bits(bits, half, hl);
    int a_rest = bits - a_theta;
    if (a_rest < 0)
        a_rest = 0;
    const double tn = theta / vq_half_pi;
    double theta_q = 0.0;
    s.code = 0ull;
    s.w_theta = 0;
    if (ANGLE32 && !__builtin_amdgcn_ballot_w64(a_theta > 31)) {
        if (a_theta > 0) {
            const unsigned c32 = vq_angle_code32(tn, a_theta);
            s.code = c32;
            s.w_theta = a_theta;
            theta_q = vq_angle_value32(c32, a_theta);
        }
    } else if (a_theta > 62) {
        if (has)
            undefined = true;
    } else if (a_theta > 0) {
        s.code = vq_angle_code(tn, a_theta);
        s.w_theta = a_theta;
        theta_q = vq_angle_value(s.code, a_theta);
    }
    if (GUARD && has && a_theta > 0 && a_theta <= 53 && pacx_quant_guard(tn, a_theta, 1e-13))
        guarded = true;
    stamp(27);
    s.a_mid = 0;
    if (theta_q != 0.0) {
        /* log2(tan(theta_q) + eps): quantised angles of up to 12 bits come from the table the caller evaluated */
        const double lt = vq_log2_tan_tabled(a_theta, theta_q) ? log2_tan(vq_log2_tan_slot(a_theta, s.code))
                                                               : vq_log2_tan(theta_q);
        s.a_mid = vq_mid_bits(a_rest, half, lt);
    }
    stamp(28);
    s.a_side = a_rest - s.a_mid;
    s.c_mid = (has && s.a_mid > 0) ? 1 : 0;
    s.c_side = (has && s.a_side > 0) ? 1 : 0;
    s.rel = wave_excl_scan_i32(s.c_mid + s.c_side, lane, s.born);
    return s;
}

/* the split `snode` gets its field, its children -- `first` and, if both exist, first + 1 -- join the store as nodes of
   depth + 1 (vectors of `half` components at tot[snode] of the next buffer) */
template <class S>
__device__ __forceinline__ void vq_split_born(const S &N, int snode, int first, int half, const VqSplit &s, int depth,
                                              bool &undefined)
{
    N.val[snode] = s.code;
    N.wid[snode] = (unsigned char)s.w_theta;
    N.kid[snode] = (typename S::index_t)first;
    N.has[snode] = (unsigned char)(s.c_mid | (s.c_side << 1));
    const int at = N.tot[snode];
    const int bd = S::bands ? N.band[snode] : 0;
#pragma unroll
    for (int c = 0; c < 2; ++c) {
        const int a = c ? s.a_side : s.a_mid;
        if (a <= 0)
            continue;
        const int id = c ? first + s.c_mid : first;
        const bool splits = a > PACX_VQ_SPLIT_BITS && depth + 1 < VQ_DEPTH;
        if (a > PACX_VQ_SPLIT_BITS && !splits)
            undefined = true;                      /* deeper than any real tree */
        N.nn[id] = (unsigned short)half;
        N.bb[id] = (unsigned short)(a > 65535 ? 65535 : a);
        N.off[id] = (unsigned short)(at + (c ? half : 0));
        N.kind[id] = splits ? 0 : 1;
        N.wid[id] = 0;
        if (S::bands)
            N.band[id] = (unsigned char)bd;
        N.has[id] = 0;
        N.kid[id] = 0;
        N.val[id] = 0ull;
    }
}

/* ---- the stream layout ------------------------------------------------------ */
/* Subtree widths and field counts bottom-up (the counts ride in nn[], lengths are not needed any more), then stream
   positions and field numbers (in off[]) top-down: the reference writes depth first -- a node's field, its mid subtree,
   its side subtree.  t: this thread's number in the team.  roots() sets pos[] and off[] of the level-0 nodes between
   the two passes.  lvl[0 .. depth + 1] is complete and visible to the team */
template <class Team, class S, class Roots>
__device__ __forceinline__ void vq_layout(const S &N, int depth, int t, Roots roots)
{
    for (int d = depth; d >= 0; --d) {
        const int b = N.lvl[d], e = N.lvl[d + 1];
        for (int j = b + t; j < e; j += Team::size) {
            const int k0 = N.kid[j], hs = N.has[j];
            int w = N.wid[j], f = (N.kind[j] == 3) ? 0 : 1;
            if (hs & 1) { w += N.tot[k0]; f += N.nn[k0]; }
            if (hs & 2) { const int k1 = k0 + (hs & 1); w += N.tot[k1]; f += N.nn[k1]; }
            N.tot[j] = (unsigned short)w;
            N.nn[j] = (unsigned short)f;
        }
        Team::sync();
    }
    roots();
    Team::sync();
    for (int d = 0; d <= depth; ++d) {
        const int b = N.lvl[d], e = N.lvl[d + 1];
        for (int j = b + t; j < e; j += Team::size) {
            const int k0 = N.kid[j], hs = N.has[j];
            int p = N.pos[j] + N.wid[j], r = N.off[j] + ((N.kind[j] == 3) ? 0 : 1);
            if (hs & 1) {
                N.pos[k0] = (unsigned short)p;
                N.off[k0] = (unsigned short)r;
                p += N.tot[k0];
                r += N.nn[k0];
            }
            if (hs & 2) {
                const int k1 = k0 + (hs & 1);
                N.pos[k1] = (unsigned short)p;
                N.off[k1] = (unsigned short)r;
            }
        }
        Team::sync();
    }
}

/* every field by its own thread; with a log, log_put(j, at, value, width) writes entry `at` of node j's band */
template <class Team, class S, class LogPut>
__device__ __forceinline__ void vq_put_fields(const S &N, int count, int t, unsigned *words, const void *log, int log_cap,
                                              LogPut log_put)
{
    for (int j = t; j < count; j += Team::size) {
        const int w = N.wid[j];
        unsigned long long v = N.val[j];
        if (w > 0 && w < 64)
            v &= (1ull << w) - 1ull;
        if (w > 0)
            vq_put_field(words, N.pos[j], v, w);
        if (log && N.kind[j] != 3 && N.off[j] < log_cap)
            log_put(j, N.off[j], v, w);
    }
}
