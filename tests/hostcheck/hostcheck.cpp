// Host build of audio-codec_amd/csrc/pacx_exact.h and vq_exact.h for the CPU test suite:
// the same source the HIP kernels compile, exported for ctypes.
#include "pacx_exact.h"
#include "pacx_vq_tables.h"
#include "vq_exact.h"

extern "C" {
double hc_pcm16_to_f64(int c) { return pacx_pcm16_to_f64(c); }
long long hc_quant_mag(double ax, int r) { return pacx_quant_mag(ax, r); }
int hc_scale_factor(double ax, int nsb, int nmb) { return pacx_scale_factor(ax, nsb, nmb); }
int hc_mantissa(double x, int scale, int nsb, int nmb) { return pacx_mantissa(x, scale, nsb, nmb); }
double hc_np_sum(const double *a, int n) { return pacx_np_sum(a, n); }
double hc_np_add_reduce(const double *a, int n)
{
    PacxPairwiseStack st;
    return pacx_np_add_reduce(n, [a](int i) { return a[i]; }, &st);
}
int hc_pairwise_stack(void) { return PACX_PAIRWISE_STACK; }
int hc_np_bufsize(void) { return PACX_NP_BUFSIZE; }
int hc_np_sum_max_n(void) { return PACX_NP_SUM_MAX_N; }
double hc_dequant_uniform(long long c, int r) { return pacx_dequant_uniform(c, r); }
int hc_mantissa_fp(double x, int scale, int nsb, int nmb) { return pacx_mantissa_fp(x, scale, nsb, nmb); }
double hc_dequantize_fp(long long m, int scale, int nsb, int nmb) { return pacx_dequantize_fp(m, scale, nsb, nmb); }
double hc_dequantize(long long m, int scale, int nsb, int nmb) { return pacx_dequantize(m, scale, nsb, nmb); }
double hc_bit_budget(double tbps, int half_n, int is_short, int lon, int nsb, int nmsb, int nb)
{ return pacx_bit_budget(tbps, half_n, is_short, lon, nsb, nmsb, nb, 0, 0); }
double hc_bit_budget_vq(double tbps, int half_n, int is_short, int lon, int nsb, int nmsb, int nb, int sbr_long)
{ return pacx_bit_budget(tbps, half_n, is_short, lon, nsb, nmsb, nb, 1, sbr_long); }
int hc_bit_alloc(double budget, int max_mant, int nb, const int32_t *n_lines, const double *smr,
                 int32_t *bits, int *hit_cap)
{ return pacx_bit_alloc(budget, max_mant, nb, n_lines, smr, bits, hit_cap); }
double hc_spl_array(double v) { return pacx_spl_array(v); }
double hc_log10_pos(double x) { return pacx_log10_pos(x); }
double hc_round_trip(double x) { return pacx_spl_of_intensity_of(x); }
double hc_exp2_lean(double y) { return pacx_exp2_lean(y); }
double hc_spl_scalar(double v) { return pacx_spl_scalar(v); }
double hc_bark(double f) { return pacx_bark(f); }
double hc_thresh_quiet(double f) { return pacx_thresh_quiet(f); }
int hc_window_kind(unsigned f) { return pacx_window_kind(f); }
int hc_quant_guard(double ax, int r, double err) { return pacx_quant_guard(ax, r, err); }
int hc_scale_guard(double ax, int nsb, int nmb, double err) { return pacx_scale_guard(ax, nsb, nmb, err); }

/* pyramid-VQ tables (pacx_vq_tables.h) */
static PacxVqHostTables g_vq;
void hc_vq_build(int l_max) { pacx_vq_build(l_max, nullptr, &g_vq); }
int hc_vq_k(int l, int bits) { return g_vq.k_of[(size_t)l * 33 + bits]; }
int hc_vq_w(int l, int bits) { return g_vq.w_of[(size_t)l * 33 + bits]; }
int hc_vq_row_len(int l) { return g_vq.row_len[l]; }
unsigned long long hc_vq_n(int l, int k) { return g_vq.n_tab[g_vq.row_off[l] + k]; }
unsigned long long hc_vq_p(int l, int k) { return g_vq.p_tab[g_vq.row_off[l] + k]; }

/* the split rule of the gain-shape coder and decoder (vq_exact.h) */
double hc_vq_half_pi(void) { return vq_half_pi; }
int hc_vq_first_bits(int bits, int l, double half_log2_l) { return vq_first_bits(bits, l, half_log2_l); }
unsigned long long hc_vq_angle_code(double tn, int a) { return vq_angle_code(tn, a); }
unsigned hc_vq_angle_code32(double tn, int a) { return vq_angle_code32(tn, a); }
double hc_vq_angle_value(unsigned long long code, int a) { return vq_angle_value(code, a); }
double hc_vq_angle_value32(unsigned code, int a) { return vq_angle_value32(code, a); }
int hc_vq_log2_tan_tabled(int a, double theta_q) { return vq_log2_tan_tabled(a, theta_q); }
int hc_vq_log2_tan_slot(int a, unsigned long long code) { return vq_log2_tan_slot(a, code); }
int hc_vq_theta_table_bits(void) { return PACX_VQ_THETA_TABLE_BITS; }
int hc_vq_mid_bits(int a_rest, int half, double lt) { return vq_mid_bits(a_rest, half, lt); }
void hc_vq_quantize_wide(double x, int n_bits, unsigned long long *hi, unsigned long long *lo)
{ vq_quantize_wide(x, n_bits, *hi, *lo); }
}
