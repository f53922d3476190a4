// chain_moments.hip -- mean and standard deviation of a device-resident chain (bisip_chain_moments_dev), and its second and
// fourth moments about a given centre (bisip_chain_central_moments_dev; bisip_amd.diagnostics: the Monte-Carlo error of the
// standard deviation), in the order of the former's second pass.
//
// The reference summarises a fit with np.mean / np.std over the flattened chain
// (src/bisip/utils.py:55-85, get_param_mean / get_param_std).  For a batch of spectra the
// chain is (n_samples, E*Wp, ndim) and lives in HBM; copying it to the host to take two
// moments per parameter would cost more than sampling it, so the two passes run here.
//
// Mapping: workgroup (e, split) sweeps a contiguous range of samples of ensemble e.  One
// sample of one ensemble is Wp*ndim contiguous doubles; the first `per*ndim` lanes of the
// workgroup (per = 256/ndim) read them as consecutive doubles, so lane t always sees
// parameter t % ndim and keeps ONE running sum -- no dynamic register indexing, coalesced
// loads.  Partial sums are combined in a fixed order (lanes, then splits): the result does
// not depend on scheduling.  Pass 0: mean.  Pass 1: sum (x - mean)^2 -> population std.
//
// The order, as include/bisip_hip.h states it and bisip_amd.chainview.ordered_moments reproduces it bit for bit:
//   splits = max(1, min(ceil(4096 / E), n / 4)); split sp takes samples [n * sp / splits, n * (sp + 1) / splits).
//   lanes = (256 / ndim) * ndim; lane t owns the doubles t, t + lanes, ... of the ensemble's Wp * ndim of a sample.
//   Four accumulators per lane from 0.0: samples in groups of four from the start of the split, for each of the lane's
//   doubles in turn sample s + j to accumulator j; the one to three samples left over to accumulator 0; the lane's sum is
//   (a0 + a1) + (a2 + a3).  Lanes q, q + ndim, ... in ascending order onto 0.0; splits in ascending order onto 0.0.
//   Pass 0 adds x; mean = sum / (double(n) * double(Wp)).  Pass 1: d = x - mean, acc = fma(d, d, acc); std = sqrt(sum /
//   count).  The workspace is counted in DOUBLES (E * splits * ndim), unlike every later *_workspace.
// Any change here changes bits that tests/test_gpu_moments.py holds: change the header and ordered_moments with it.
#include "chain.h"

using namespace bisip;
using namespace bisip::host;

struct MomentArgs {
    const double *chain;     // first used sample
    long long n_samples;     // used samples
    long long sample_stride; // doubles between consecutive used samples
    long long E, Wp;
    int ndim, splits;
    double *mean, *std;      // (E, ndim)
    double *partial;         // (E, splits, ndim) workspace
};

template <int PASS>
__global__ __launch_bounds__(256) void k_moments_partial(const MomentArgs a)
{
    __shared__ double part[256];
    const int e = blockIdx.x, sp = blockIdx.y;
    const int per = 256 / a.ndim, lanes = per * a.ndim;
    const int t = threadIdx.x;
    const int q = t % a.ndim;
    const long long s0 = a.n_samples * sp / a.splits, s1 = a.n_samples * (sp + 1) / a.splits;
    const long long len = a.Wp * a.ndim;  // doubles of this ensemble per sample
    const double *base = a.chain + (long long)e * len;
    const double m = PASS ? a.mean[(long long)e * a.ndim + q] : 0.0;
    // four samples in flight per lane (independent running sums, combined in a fixed order): a
    // single dependent stream of loads per lane left the sweep latency-bound once the chain no
    // longer fits the last-level cache (1.8 GB: 0.11 TB/s)
    double acc4[4] = {0.0, 0.0, 0.0, 0.0};
    auto add = [&](double &acc, double x) { if (PASS) { const double d = x - m; acc = fma(d, d, acc); } else acc += x; };
    if (t < lanes) {
        long long s = s0;
        for (; s + 4 <= s1; s += 4) {
            const double *p = base + s * a.sample_stride;
            for (long long i = t; i < len; i += lanes) {  // i % ndim == q for every i
                const double x0 = __builtin_nontemporal_load(p + i), x1 = __builtin_nontemporal_load(p + a.sample_stride + i);
                const double x2 = __builtin_nontemporal_load(p + 2 * a.sample_stride + i), x3 = __builtin_nontemporal_load(p + 3 * a.sample_stride + i);
                add(acc4[0], x0); add(acc4[1], x1); add(acc4[2], x2); add(acc4[3], x3);
            }
        }
        for (; s < s1; ++s) {
            const double *p = base + s * a.sample_stride;
            for (long long i = t; i < len; i += lanes) add(acc4[0], __builtin_nontemporal_load(p + i));
        }
    }
    const double acc = (acc4[0] + acc4[1]) + (acc4[2] + acc4[3]);
    part[t] = acc;
    __syncthreads();
    if (t < a.ndim) {
        double sum = 0.0;
        for (int k = 0; k < per; ++k) sum += part[k * a.ndim + t];
        a.partial[((long long)e * a.splits + sp) * a.ndim + t] = sum;
    }
}

template <int PASS>
__global__ __launch_bounds__(256) void k_moments_finish(const MomentArgs a)
{
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;  // (e, q)
    if (idx >= a.E * a.ndim) return;
    const long long e = idx / a.ndim;
    const int q = (int)(idx % a.ndim);
    double sum = 0.0;
    for (int sp = 0; sp < a.splits; ++sp) sum += a.partial[(e * a.splits + sp) * a.ndim + q];
    const double cnt = (double)a.n_samples * (double)a.Wp;
    if (PASS) a.std[idx] = sqrt(sum / cnt);
    else a.mean[idx] = sum / cnt;
}

// bisip_chain_central_moments_dev: the means of (x - c)^2 and (x - c)^4 about a given centre c (E, ndim), in the order of
// pass 1 above -- the same splits, lanes, four accumulators per lane (here four per moment) and ascending combination.
// Per value d = x - c and q = d * d round once each; acc2 = fma(d, d, acc2), acc4 = fma(q, q, acc4).
struct CentralArgs {
    const double *chain;
    long long n_samples, sample_stride, E, Wp;
    int ndim, splits;
    const double *center;    // (E, ndim)
    double *m2, *m4;         // (E, ndim)
    double *partial;         // (2, E, splits, ndim) workspace: the sums of squares, then of fourth powers
};

__global__ __launch_bounds__(256) void k_central_partial(const CentralArgs a)
{
    __shared__ double part2[256], part4[256];
    const int e = blockIdx.x, sp = blockIdx.y;
    const int per = 256 / a.ndim, lanes = per * a.ndim;
    const int t = threadIdx.x;
    const int q = t % a.ndim;
    const long long s0 = a.n_samples * sp / a.splits, s1 = a.n_samples * (sp + 1) / a.splits;
    const long long len = a.Wp * a.ndim;
    const double *base = a.chain + (long long)e * len;
    const double c = a.center[(long long)e * a.ndim + q];
    double a2[4] = {0.0, 0.0, 0.0, 0.0}, a4[4] = {0.0, 0.0, 0.0, 0.0};
    auto add = [&](double &s2, double &s4, double x) {
        const double d = x - c, dd = d * d;
        s2 = fma(d, d, s2);
        s4 = fma(dd, dd, s4);
    };
    if (t < lanes) {
        long long s = s0;
        for (; s + 4 <= s1; s += 4) {
            const double *p = base + s * a.sample_stride;
            for (long long i = t; i < len; i += lanes) {
                const double x0 = __builtin_nontemporal_load(p + i), x1 = __builtin_nontemporal_load(p + a.sample_stride + i);
                const double x2 = __builtin_nontemporal_load(p + 2 * a.sample_stride + i), x3 = __builtin_nontemporal_load(p + 3 * a.sample_stride + i);
                add(a2[0], a4[0], x0); add(a2[1], a4[1], x1); add(a2[2], a4[2], x2); add(a2[3], a4[3], x3);
            }
        }
        for (; s < s1; ++s) {
            const double *p = base + s * a.sample_stride;
            for (long long i = t; i < len; i += lanes) add(a2[0], a4[0], __builtin_nontemporal_load(p + i));
        }
    }
    part2[t] = (a2[0] + a2[1]) + (a2[2] + a2[3]);
    part4[t] = (a4[0] + a4[1]) + (a4[2] + a4[3]);
    __syncthreads();
    if (t < a.ndim) {
        double sum2 = 0.0, sum4 = 0.0;
        for (int k = 0; k < per; ++k) {
            sum2 += part2[k * a.ndim + t];
            sum4 += part4[k * a.ndim + t];
        }
        const long long at = ((long long)e * a.splits + sp) * a.ndim + t;
        a.partial[at] = sum2;
        a.partial[a.E * a.splits * a.ndim + at] = sum4;
    }
}

__global__ __launch_bounds__(256) void k_central_finish(const CentralArgs a)
{
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;  // (e, q)
    if (idx >= a.E * a.ndim) return;
    const long long e = idx / a.ndim;
    const int q = (int)(idx % a.ndim);
    const double *p4 = a.partial + a.E * a.splits * a.ndim;
    double sum2 = 0.0, sum4 = 0.0;
    for (int sp = 0; sp < a.splits; ++sp) {
        sum2 += a.partial[(e * a.splits + sp) * a.ndim + q];
        sum4 += p4[(e * a.splits + sp) * a.ndim + q];
    }
    const double cnt = (double)a.n_samples * (double)a.Wp;
    a.m2[idx] = sum2 / cnt;
    a.m4[idx] = sum4 / cnt;
}

static int moment_splits(int64_t n_samples, int64_t E)
{
    // enough workgroups to fill the chip (256 CUs x 16), at least four samples each
    int64_t s = (4096 + E - 1) / E;
    if (s > n_samples / 4) s = n_samples / 4;
    return (int)(s < 1 ? 1 : s);
}

// E: grid dimension x of the partial sums.  Neither n nor Wp is capped: the kernels index both in 64 bits.
static int check_moments_chain(const ChainShape &s) { return check_chain(s, 1, NO_CAP, GRID_MAX, NO_CAP); }

extern "C" {

int64_t bisip_chain_moments_workspace(int64_t n_samples, int64_t n_ensembles, int ndim)
{
    if (n_samples < 1 || n_ensembles < 1 || ndim < 1) return 0;
    return n_ensembles * moment_splits(n_samples, n_ensembles) * (int64_t)ndim;
}

int bisip_chain_moments_dev(const double *d_chain, int64_t n_samples, int64_t sample_stride,
                            int64_t n_ensembles, int64_t walkers_per_ensemble, int ndim,
                            double *d_mean, double *d_std, double *d_work, void *stream)
{
    if (!d_chain || !d_mean || !d_std || !d_work) return fail(BISIP_EINVAL, "null argument");
    BISIP_TRY(check_moments_chain({n_samples, sample_stride, n_ensembles, walkers_per_ensemble, ndim}));
    MomentArgs a;
    a.chain = d_chain; a.n_samples = n_samples; a.sample_stride = sample_stride;
    a.E = n_ensembles; a.Wp = walkers_per_ensemble; a.ndim = ndim;
    a.splits = moment_splits(n_samples, n_ensembles);
    a.mean = d_mean; a.std = d_std; a.partial = d_work;
    const dim3 grid((unsigned)n_ensembles, (unsigned)a.splits);
    const dim3 fin((unsigned)((n_ensembles * ndim + 255) / 256));
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_moments_partial<0>, grid, dim3(256), 0, st, a);
    hipLaunchKernelGGL(k_moments_finish<0>, fin, dim3(256), 0, st, a);
    hipLaunchKernelGGL(k_moments_partial<1>, grid, dim3(256), 0, st, a);
    hipLaunchKernelGGL(k_moments_finish<1>, fin, dim3(256), 0, st, a);
    HIP_TRY(hipGetLastError());
    return BISIP_OK;
}

int64_t bisip_chain_central_moments_workspace(int64_t n_samples, int64_t n_ensembles, int ndim)
{
    return 2 * bisip_chain_moments_workspace(n_samples, n_ensembles, ndim);
}

int bisip_chain_central_moments_dev(const double *d_chain, int64_t n_samples, int64_t sample_stride,
                                    int64_t n_ensembles, int64_t walkers_per_ensemble, int ndim,
                                    const double *d_center, double *d_m2, double *d_m4, double *d_work, void *stream)
{
    if (!d_chain || !d_center || !d_m2 || !d_m4 || !d_work) return fail(BISIP_EINVAL, "null argument");
    BISIP_TRY(check_moments_chain({n_samples, sample_stride, n_ensembles, walkers_per_ensemble, ndim}));
    CentralArgs a;
    a.chain = d_chain; a.n_samples = n_samples; a.sample_stride = sample_stride;
    a.E = n_ensembles; a.Wp = walkers_per_ensemble; a.ndim = ndim;
    a.splits = moment_splits(n_samples, n_ensembles);
    a.center = d_center; a.m2 = d_m2; a.m4 = d_m4; a.partial = d_work;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(k_central_partial, dim3((unsigned)n_ensembles, (unsigned)a.splits), dim3(256), 0, st, a);
    hipLaunchKernelGGL(k_central_finish, dim3((unsigned)((n_ensembles * ndim + 255) / 256)), dim3(256), 0, st, a);
    HIP_TRY(hipGetLastError());
    return BISIP_OK;
}

}  // extern "C"
