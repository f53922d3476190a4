// chain_rtd_descriptors.hip -- the relaxation descriptors of every used sample of a device-resident
// PolynomialDecomposition chain: the relaxation time and height of the RTD's peak and the cumulative relaxation times
// log_tau_q at which a fraction q of the clipped RTD's sum has accumulated (bisip_rtd_descriptors_dev), and the same
// rows on the host (bisip_rtd_descriptors_host: host pointers, launches nothing), so that the kernel's bits can be
// compared with the host's.  The arithmetic of a row is rtd_descriptor_row<ND> (rtd_descriptors.h) for both; the
// definitions are in the module docstring of bisip_amd/decomposition.py.  The output is a chain of ndim = 2 + n_q
// that the moments, percentiles and HDI summarise.
#include "chain.h"
#include "rtd_descriptors.h"

using namespace bisip;
using namespace bisip::host;

namespace {

struct RtdDescriptorArgs {
    const double *chain;
    long long n_samples, sample_stride;
    unsigned rows;           // rows of one sample (E*Wp < 2^31)
    int L, nq;
    double *out;             // (n_samples, E*Wp, 2 + nq)
};

// Grid as k_rtd_integrals (chain_rtd.hip): thread x = row r = e*Wp + w of the samples blockIdx.y, blockIdx.y +
// gridDim.y, ...; 32-bit index arithmetic within a sample.  x = log_tau (L,) and q (nq,) are the same for every lane;
// they are kernel arguments of their own, const and __restrict__, which is what lets the compiler prove that the
// stores to out leave them alone and read them through scalar loads.  The two passes over l evaluate Horner twice: L
// is a run-time value, so the m_l have no registers to stay in.
template <int ND>
__global__ __launch_bounds__(256) void k_rtd_descriptors(const RtdDescriptorArgs a, const double *__restrict__ x,
                                                         const double *__restrict__ q)
{
    const unsigned r = blockIdx.x * 256u + threadIdx.x;
    if (r >= a.rows) return;
    const int K = 2 + a.nq;
    for (long long s = blockIdx.y; s < a.n_samples; s += gridDim.y) {
        const double *__restrict__ row = a.chain + s * a.sample_stride + (long long)r * ND;
        double th[ND];
#pragma unroll
        for (int p = 0; p < ND; ++p) th[p] = __builtin_nontemporal_load(row + p);
        double o[2 + RTD_MAX_FRACTIONS];
        rtd_descriptor_row<ND>(th, x, a.L, q, a.nq, o);
        double *__restrict__ dst = a.out + (s * a.rows + r) * K;
#pragma unroll
        for (int k = 0; k < 2 + RTD_MAX_FRACTIONS; ++k)
            if (k < K) dst[k] = o[k];
    }
}

struct RtdDescriptorLaunchArgs {
    RtdDescriptorArgs row;
    const double *log_tau, *q;
};

template <int ND>
struct DescriptorsLaunch {
    static void run(dim3 grid, hipStream_t st, const RtdDescriptorLaunchArgs &a)
    {
        hipLaunchKernelGGL(k_rtd_descriptors<ND>, grid, dim3(256), 0, st, a.row, a.log_tau, a.q);
    }
};

// the argument checks of bisip_rtd_columns_dev, plus 1 <= n_q <= 8
int check_descriptor_args(const void *chain, const void *log_tau, const void *q, const void *out, int64_t n_samples,
                          int64_t sample_stride, int64_t n_ensembles, int64_t walkers_per_ensemble, int ndim, int n_tau,
                          int n_q)
{
    if (!chain || !log_tau || !q || !out) return fail(BISIP_EINVAL, "null argument");
    if (n_tau < 1) return fail(BISIP_EINVAL, "n_tau=%d", n_tau);
    if (n_q < 1 || n_q > RTD_MAX_FRACTIONS) return fail(BISIP_EINVAL, "n_q=%d out of range [1, %d]", n_q, RTD_MAX_FRACTIONS);
    const ChainShape s{n_samples, sample_stride, n_ensembles, walkers_per_ensemble, ndim};
    BISIP_TRY(check_chain(s, 2, NO_CAP, NO_CAP, NO_CAP));      // (as bisip_rtd_integrals_dev: the rows come after the stride)
    return check_rows(s);
}

}  // namespace

extern "C" {

int bisip_rtd_descriptors_dev(const double *d_chain, int64_t n_samples, int64_t sample_stride, int64_t n_ensembles,
                              int64_t walkers_per_ensemble, int ndim, const double *d_log_tau, int n_tau,
                              const double *d_q, int n_q, double *d_out, void *stream)
{
    int rc = check_descriptor_args(d_chain, d_log_tau, d_q, d_out, n_samples, sample_stride, n_ensembles,
                                   walkers_per_ensemble, ndim, n_tau, n_q);
    if (rc != BISIP_OK) return rc;
    const int64_t rows = n_ensembles * walkers_per_ensemble;
    const RtdDescriptorLaunchArgs a{{d_chain, n_samples, sample_stride, (unsigned)rows, n_tau, n_q, d_out}, d_log_tau, d_q};
    // x: the rows of one sample; y: samples, a grid-stride loop beyond 65535
    const dim3 grid((unsigned)((rows + 255) / 256), (unsigned)(n_samples < 65535 ? n_samples : 65535));
    return launch_by_ndim<DescriptorsLaunch>(ndim, grid, (hipStream_t)stream, a);
}

int bisip_rtd_descriptors_host(const double *chain, int64_t n_samples, int64_t sample_stride, int64_t n_ensembles,
                               int64_t walkers_per_ensemble, int ndim, const double *log_tau, int n_tau,
                               const double *q, int n_q, double *out)
{
    int rc = check_descriptor_args(chain, log_tau, q, out, n_samples, sample_stride, n_ensembles, walkers_per_ensemble,
                                   ndim, n_tau, n_q);
    if (rc != BISIP_OK) return rc;
    if (!rtd_descriptor_rows_host_by_ndim<BISIP_MAX_NDIM>(ndim, chain, n_samples, sample_stride,
                                                          n_ensembles * walkers_per_ensemble, log_tau, n_tau, q, n_q, out))
        return fail(BISIP_EINVAL, "no row function of ndim=%d", ndim);      // (check_descriptor_args has checked ndim)
    return BISIP_OK;
}

}  // extern "C"
