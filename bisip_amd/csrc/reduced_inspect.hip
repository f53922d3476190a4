// reduced_inspect.hip -- host-only entry points that make the QR-reduced kernels' bits checkable from outside:
// bisip_reduced_emulate (the host emulation of logprob_row_reduced<P, COMP>, host_emulate.inc: chi2_kernel, then the
// prior) and bisip_ctx_reduced_operands (a spectrum's entry of a tier's image -- host.h: ReducedLayout -- which is
// what a lone spectrum's kernel argument is copied from and what the device array is uploaded from).  Nothing here
// launches anything or changes a context.  tests/test_gpu_reduced_bits.py holds every instantiation and launch route of
// logprob_row_reduced (kernels.h) to the emulation bit for bit on these operands: reorder a sum in the kernel and
// host_emulate.inc has to follow, and the other way round.
#include "host.h"

using namespace bisip;
using namespace bisip::host;

int bisip_ctx_reduced_operands(const bisip_ctx *c, int64_t spectrum, int tier, double *R, float *Rlo, double *bhat,
                               double *e, double *elo, double *rest, double *lconst, int *runs)
{
    if (!c || !R || !bhat || !e || !elo || !rest || !lconst || !runs) return fail(BISIP_EINVAL, "null argument");
    if (c->model_id != BISIP_MODEL_POLYDECOMP || c->reduced.empty())
        return fail(BISIP_EINVAL, "only PolynomialDecomposition contexts have a QR-reduced form");
    if (tier != 0 && tier != 1) return fail(BISIP_EINVAL, "tier=%d is neither 0 (plain) nor 1 (compensated)", tier);
    if (tier == 1 && !Rlo) return fail(BISIP_EINVAL, "the compensated tier needs Rlo");
    if (spectrum < 0 || spectrum >= c->E) return fail(BISIP_EINVAL, "spectrum=%lld out of range", (long long)spectrum);
    const bisip_ctx::ReducedTier &T = c->red[tier];
    const size_t s = (size_t)spectrum;
    if (!T.valid || T.done.size() <= s || !T.done[s])
        return fail(BISIP_EINVAL, "tier %d holds no operands of spectrum %lld under the current prior box", tier, (long long)spectrum);
    const ReducedLayout L(c->P + 2);
    const size_t per = L.doubles(tier);
    if (T.image.size() != per * (size_t)c->E) return fail(BISIP_EHIP, "internal: tier %d has no image of this layout", tier);
    L.unpack(tier, &T.image[per * s], R, Rlo, bhat, e, elo, rest);
    *lconst = c->E > 1 ? c->reduced[s].lconst : c->lconst;
    *runs = running_tier(c, s) == tier;
    return BISIP_OK;
}

int bisip_reduced_emulate(int n, int comp, const double *R, const float *Rlo, const double *bhat, const double *e,
                          const double *elo, double rest, double lconst, const double *lo, const double *hi,
                          const double *theta, int64_t W, double *out)
{
    if (!R || !bhat || !e || !lo || !hi) return fail(BISIP_EINVAL, "null argument");
    if (n < 2 || n > BISIP_MAX_POLY_DEG + 2) return fail(BISIP_EINVAL, "n=%d out of range [2, %d]", n, BISIP_MAX_POLY_DEG + 2);
    if (comp != 0 && comp != 1) return fail(BISIP_EINVAL, "comp=%d is neither 0 nor 1", comp);
    if (comp && (!Rlo || !elo)) return fail(BISIP_EINVAL, "the compensated form needs Rlo and elo");
    if (W < 0) return fail(BISIP_EINVAL, "W=%lld < 0", (long long)W);
    if (W > 0 && (!theta || !out)) return fail(BISIP_EINVAL, "null buffer");
    constexpr int MAXN = BISIP_MAX_POLY_DEG + 2;
    double Rfull[MAXN * MAXN];                   // the (n,n) layout chi2_kernel reads
    float Rlo_full[MAXN * MAXN];
    ReducedLayout(n).expand(R, comp ? Rlo : nullptr, Rfull, Rlo_full);
    for (int64_t w = 0; w < W; ++w) {
        const double *th = theta + w * n;
        bool inside = true;                      // kernels.h: in_prior -- strict, NaN -> false
        for (int q = 0; q < n; ++q) inside = inside && (lo[q] < th[q]) && (th[q] < hi[q]);
        const double chi2 = reduced_chi2_kernel(n, Rfull, comp ? Rlo_full : nullptr, bhat, e, elo, rest, th, comp != 0);
        out[w] = inside ? std::fma(-0.5, chi2, lconst) : -INFINITY;
    }
    return BISIP_OK;
}
