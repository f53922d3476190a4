// chain_modes.hip -- the modes of every used sample of a device-resident PeltonColeCole chain put in order, with the
// per-mode descriptors of the ordered row: the total chargeability, the Cole-Cole time constant and the phase-peak
// relaxation time of every mode (bisip_mode_order_dev), and the same rows on the host (bisip_mode_order_host: host
// pointers, launches nothing), so that the kernel's bits can be compared with the host's.  The arithmetic of a row is
// mode_order_row<K> (mode_order.h) for both; the definitions are in the module docstring of bisip_amd/modes.py.  The
// ordered rows are a chain of ndim = 1 + 3K and the descriptors one of ndim = 1 + 2K that the moments, percentiles and
// HDI summarise.
#include "chain_check.h"
#include "host.h"
#include "mode_order.h"

using namespace bisip;
using namespace bisip::host;

namespace {

struct ModeOrderArgs {
    const double *chain;
    long long n_samples, sample_stride;
    unsigned rows;           // rows of one sample (E*Wp < 2^31)
    int key_group;
    double *ordered;         // (n_samples, E*Wp, 1 + 3K) or null
    double *desc;            // (n_samples, E*Wp, 1 + 2K) or null
    unsigned char *moved;    // (n_samples, E*Wp) or null
};

// Grid as k_rtd_descriptors (chain_rtd_descriptors.hip): thread x = row r = e*Wp + w of the samples blockIdx.y,
// blockIdx.y + gridDim.y, ...; 32-bit index arithmetic within a sample.  Which outputs are asked for is the same for
// every lane: an output that is not asked for costs no store, and without the descriptors no log1p is taken.
template <int K>
__global__ __launch_bounds__(256) void k_mode_order(const ModeOrderArgs a)
{
    constexpr int ND = 1 + 3 * K, NDESC = 1 + 2 * K;
    const unsigned r = blockIdx.x * 256u + threadIdx.x;
    if (r >= a.rows) return;
    for (long long s = blockIdx.y; s < a.n_samples; s += gridDim.y) {
        const double *__restrict__ row = a.chain + s * a.sample_stride + (long long)r * ND;
        double th[ND];
#pragma unroll
        for (int p = 0; p < ND; ++p) th[p] = __builtin_nontemporal_load(row + p);
        double o[ND], d[NDESC];
        const bool mv = mode_order_row<K>(th, a.key_group, o, d, a.desc != nullptr);
        const long long at = s * a.rows + r;
        if (a.ordered) {
            double *__restrict__ dst = a.ordered + at * ND;
#pragma unroll
            for (int k = 0; k < ND; ++k) dst[k] = o[k];
        }
        if (a.desc) {
            double *__restrict__ dst = a.desc + at * NDESC;
#pragma unroll
            for (int k = 0; k < NDESC; ++k) dst[k] = d[k];
        }
        if (a.moved) a.moved[at] = mv ? 1 : 0;
    }
}

// the chain-shape checks of check_descriptor_args (chain_rtd_descriptors.hip), the mode count, the key group and the
// outputs
int check_mode_order_args(const void *chain, int64_t n_samples, int64_t sample_stride, int64_t n_ensembles,
                          int64_t walkers_per_ensemble, int n_modes, int key_group, const void *ordered, const void *desc,
                          const void *moved)
{
    if (!chain) return fail(BISIP_EINVAL, "null argument");
    if (!ordered && !desc && !moved) return fail(BISIP_EINVAL, "no output asked for");
    if (n_modes < 1 || n_modes > BISIP_MAX_MODES)
        return fail(BISIP_EINVAL, "n_modes=%d out of range [1, %d]", n_modes, BISIP_MAX_MODES);
    if (key_group < MODE_KEY_M || key_group > MODE_KEY_C)
        return fail(BISIP_EINVAL, "key_group=%d (0: m, 1: log_tau, 2: c)", key_group);
    const ChainShape s{n_samples, sample_stride, n_ensembles, walkers_per_ensemble, 1 + 3 * n_modes};     // (ndim: n_modes is checked)
    BISIP_TRY(check_counts(s, NO_CAP, NO_CAP, NO_CAP));
    BISIP_TRY(check_stride(s));
    return check_rows(s);
}

}  // namespace

extern "C" {

int bisip_mode_order_dev(const double *d_chain, int64_t n_samples, int64_t sample_stride, int64_t n_ensembles,
                         int64_t walkers_per_ensemble, int n_modes, int key_group, double *d_ordered, double *d_desc,
                         unsigned char *d_moved, void *stream)
{
    int rc = check_mode_order_args(d_chain, n_samples, sample_stride, n_ensembles, walkers_per_ensemble, n_modes, key_group,
                                   d_ordered, d_desc, d_moved);
    if (rc != BISIP_OK) return rc;
    const int64_t rows = n_ensembles * walkers_per_ensemble;
    const ModeOrderArgs a{d_chain, n_samples, sample_stride, (unsigned)rows, key_group, d_ordered, d_desc, d_moved};
    // x: the rows of one sample; y: samples, a grid-stride loop beyond 65535
    const dim3 grid((unsigned)((rows + 255) / 256), (unsigned)(n_samples < 65535 ? n_samples : 65535));
    return with_mode_count(n_modes, "mode-order", [&](auto k) {
        hipLaunchKernelGGL(k_mode_order<decltype(k)::value>, grid, dim3(256), 0, (hipStream_t)stream, a);
        HIP_TRY(hipGetLastError());
        return (int)BISIP_OK;
    });
}

int bisip_mode_order_host(const double *chain, int64_t n_samples, int64_t sample_stride, int64_t n_ensembles,
                          int64_t walkers_per_ensemble, int n_modes, int key_group, double *ordered, double *desc,
                          unsigned char *moved)
{
    int rc = check_mode_order_args(chain, n_samples, sample_stride, n_ensembles, walkers_per_ensemble, n_modes, key_group,
                                   ordered, desc, moved);
    if (rc != BISIP_OK) return rc;
    return with_mode_count(n_modes, "mode-order", [&](auto k) {
        mode_order_rows_host<decltype(k)::value>(chain, n_samples, sample_stride, n_ensembles * walkers_per_ensemble,
                                                 key_group, ordered, desc, moved);
        return (int)BISIP_OK;
    });
}

}  // extern "C"
