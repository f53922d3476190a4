// chain_rtd.hip -- PolynomialDecomposition's relaxation time distribution and integrating parameters of every used
// sample of a device-resident chain (bisip_rtd_integrals_dev, bisip_rtd_columns_dev); their outputs are chains and
// columns that the moments and percentiles summarise.
//
// The relaxation time distribution m_l = sum_p a_p log_tau_l^p of every used sample
// (theta = (r0, a_0, ..., a_P), ascending powers; P = ndim - 2) and the integrating parameters taken from it --
// docs/tutorials/decomposition.ipynb, get_m (np.sum(m) = total_m) and the RTD plots after it.
//   * k_rtd_integrals: m_total = sum_p a_p S_p and sum_l m_l log_tau_l = sum_p a_p S_{p+1}, where S_k =
//     sum_l log_tau_l^k comes from the host (long double, rounded once): O(P) per sample, the chain read once.
//     Writes (m_total, log_tau_mean, m_norm) per sample as a chain of ndim = 3.
//   * k_rtd_columns: m_l of every used sample, one column per (ensemble, l), Horner with fma; consecutive lanes
//     take consecutive walkers, so every column write is coalesced.
// Explicit fma() only (the library builds with -ffp-contract=off); plain IEEE division, no clamping.
#include "chain.h"

using namespace bisip;
using namespace bisip::host;

namespace {

struct RtdIntegralArgs {
    const double *chain;
    long long n_samples, sample_stride;
    unsigned rows, Wp;       // rows of one sample (E*Wp < 2^31), walkers per ensemble
    const double *S;         // (ndim,) S_0 ... S_{P+1}
    const double *norm;      // (E,) norm_factor of every ensemble
    double *out;             // (n_samples, E*Wp, 3)
};

// Grid (rows of a sample / 256, samples): thread x = row r = e*Wp + w of the samples blockIdx.y, blockIdx.y +
// gridDim.y, ...; 32-bit index arithmetic within a sample.  ND = ndim.
template <int ND>
__global__ __launch_bounds__(256) void k_rtd_integrals(const RtdIntegralArgs a)
{
    const unsigned r = blockIdx.x * 256u + threadIdx.x;
    if (r >= a.rows) return;
    const double nf = a.norm[r / a.Wp];
    for (long long s = blockIdx.y; s < a.n_samples; s += gridDim.y) {
        const double *__restrict__ row = a.chain + s * a.sample_stride + (long long)r * ND;
        double th[ND];
#pragma unroll
        for (int q = 0; q < ND; ++q) th[q] = __builtin_nontemporal_load(row + q);
        double den = th[1] * a.S[0], num = th[1] * a.S[1];
#pragma unroll
        for (int p = 1; p < ND - 1; ++p) {
            den = fma(th[1 + p], a.S[p], den);
            num = fma(th[1 + p], a.S[p + 1], num);
        }
        double *o = a.out + (s * a.rows + r) * 3;
        o[0] = den;
        o[1] = num / den;
        o[2] = den / (th[0] * nf);
    }
}

struct RtdColumnArgs {
    const double *chain;
    long long n_samples, sample_stride;
    unsigned rows, Wp;       // rows of one sample in the pass (k*Wp < 2^31), walkers per ensemble
    long long e0;            // ensembles [e0, e0 + k) of the chain
    int L;
    const double *log_tau;   // (L,)
    double *cols;            // (k*L, n_samples*Wp)
};

// Grid as k_rtd_integrals: thread x = row r = e*Wp + w of the pass (e within the pass); m_l of its row for every l
template <int ND>
__global__ __launch_bounds__(256) void k_rtd_columns(const RtdColumnArgs a)
{
    const unsigned r = blockIdx.x * 256u + threadIdx.x;
    if (r >= a.rows) return;
    const unsigned e = r / a.Wp, w = r - e * a.Wp;
    constexpr int P = ND - 2;
    const long long n = a.n_samples * a.Wp;
    const double *__restrict__ first = a.chain + ((a.e0 + e) * (long long)a.Wp + w) * ND;
    double *__restrict__ col0 = a.cols + (long long)e * a.L * n + w;
    for (long long s = blockIdx.y; s < a.n_samples; s += gridDim.y) {
        const double *__restrict__ row = first + s * a.sample_stride;
        double c[P + 1];
#pragma unroll
        for (int p = 0; p <= P; ++p) c[p] = __builtin_nontemporal_load(row + 1 + p);
        double *__restrict__ dst = col0 + s * a.Wp;
        for (int l = 0; l < a.L; ++l) {
            const double x = a.log_tau[l];
            double m = c[P];
#pragma unroll
            for (int p = P - 1; p >= 0; --p) m = fma(m, x, c[p]);
            dst[(long long)l * n] = m;
        }
    }
}

template <int ND>
struct IntegralsLaunch {
    static void run(dim3 grid, hipStream_t st, const RtdIntegralArgs &a)
    {
        hipLaunchKernelGGL(k_rtd_integrals<ND>, grid, dim3(256), 0, st, a);
    }
};

template <int ND>
struct ColumnsLaunch {
    static void run(dim3 grid, hipStream_t st, const RtdColumnArgs &a)
    {
        hipLaunchKernelGGL(k_rtd_columns<ND>, grid, dim3(256), 0, st, a);
    }
};

// x: the rows of one sample; y: samples, a grid-stride loop beyond 65535
dim3 rtd_grid(int64_t rows, int64_t n_samples)
{
    return dim3((unsigned)((rows + 255) / 256), (unsigned)(n_samples < 65535 ? n_samples : 65535));
}

}  // namespace

extern "C" {

int bisip_rtd_integrals_dev(const double *d_chain, int64_t n_samples, int64_t sample_stride, int64_t n_ensembles,
                            int64_t walkers_per_ensemble, int ndim, const double *d_power_sums,
                            const double *d_norm_factor, double *d_out, void *stream)
{
    if (!d_chain || !d_power_sums || !d_norm_factor || !d_out) return fail(BISIP_EINVAL, "null argument");
    // no count is capped as a bad shape: the rows of a sample beyond 32 bits are unsupported, and reported after the stride
    const ChainShape s{n_samples, sample_stride, n_ensembles, walkers_per_ensemble, ndim};
    BISIP_TRY(check_chain(s, 2, NO_CAP, NO_CAP, NO_CAP));
    BISIP_TRY(check_rows(s));
    const int64_t rows = n_ensembles * walkers_per_ensemble;
    const RtdIntegralArgs a{d_chain, n_samples, sample_stride, (unsigned)rows, (unsigned)walkers_per_ensemble,
                            d_power_sums, d_norm_factor, d_out};
    return launch_by_ndim<IntegralsLaunch>(ndim, rtd_grid(rows, n_samples), (hipStream_t)stream, a);
}

int bisip_rtd_columns_dev(const double *d_chain, int64_t n_samples, int64_t sample_stride, int64_t n_ensembles,
                          int64_t walkers_per_ensemble, int ndim, int64_t first_ensemble, int64_t count,
                          const double *d_log_tau, int n_tau, double *d_cols, void *stream)
{
    if (!d_chain || !d_log_tau || !d_cols) return fail(BISIP_EINVAL, "null argument");
    if (n_tau < 1) return fail(BISIP_EINVAL, "n_tau=%d", n_tau);
    if (first_ensemble < 0 || count < 1 || first_ensemble + count > n_ensembles)
        return fail(BISIP_EINVAL, "ensembles [%lld, %lld) outside [0, %lld)", (long long)first_ensemble,
                    (long long)(first_ensemble + count), (long long)n_ensembles);
    // the rows of the whole sample come before the shape here, and cover the count * Wp rows the kernel numbers
    const ChainShape s{n_samples, sample_stride, n_ensembles, walkers_per_ensemble, ndim};
    BISIP_TRY(check_rows(s));
    BISIP_TRY(check_chain(s, 2, NO_CAP, NO_CAP, NO_CAP));
    const int64_t rows = count * walkers_per_ensemble;
    const RtdColumnArgs a{d_chain, n_samples, sample_stride, (unsigned)rows, (unsigned)walkers_per_ensemble,
                          first_ensemble, n_tau, d_log_tau, d_cols};
    return launch_by_ndim<ColumnsLaunch>(ndim, rtd_grid(rows, n_samples), (hipStream_t)stream, a);
}

}  // extern "C"
