// reduced_inspect.hip -- host-only entry points that make the QR-reduced kernels' bits checkable from outside:
// bisip_reduced_emulate (the host emulation of logprob_row_reduced<P, COMP>, host_emulate.inc: chi2_kernel, then the
// prior) and bisip_ctx_reduced_operands (the host copies of the operands the device holds).  Nothing here launches
// anything or changes a context.  tests/test_gpu_reduced_bits.py holds every instantiation and launch route of
// logprob_row_reduced (kernels.h) to the emulation bit for bit on these operands: reorder a sum in the kernel and
// host_emulate.inc has to follow, and the other way round.
#include "host.h"

using namespace bisip;
using namespace bisip::host;

namespace {

// a device image of a tier's operands exists for every tier of a batch and for a lone spectrum's compensated tier
// from degree 6 on (bisip_hip.hip: recenter_reduced)
bool has_image(const bisip_ctx *c, int tier)
{
    return c->E > 1 || (tier == 1 && c->P >= REDUCED_COMP_MEMORY_OPERANDS_FROM);
}

// doubles of one spectrum's entry of a tier's image, sizeof(ReducedArgs<P, COMP>) / 8: [Rlo |] R | bhat | e | elo | rest,
// the low word as floats, an even number of them (*lo_floats)
size_t image_doubles(int n, int tier, size_t *lo_floats)
{
    const size_t tri = (size_t)n * (n + 1) / 2;
    *lo_floats = (tri + 1) & ~(size_t)1;
    return tri + 3 * (size_t)n + 1 + (tier == 1 ? *lo_floats / 2 : 0);
}
static_assert(sizeof(ReducedArgs<5, false>) == 8 * (28 + 21 + 1) && sizeof(ReducedArgs<5, true>) == 8 * (28 + 21 + 1 + 14) &&
              sizeof(ReducedArgs<10, true>) == 8 * (78 + 36 + 1 + 39), "image_doubles is the layout of ReducedArgs");

}  // namespace

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
    const int n = c->P + 2;
    const size_t tri = (size_t)n * (n + 1) / 2;
    size_t lo_floats = 0;
    const size_t per = image_doubles(n, tier, &lo_floats);
    if (has_image(c, tier)) {                    // what recenter_reduced uploads
        if (T.image.size() != per * (size_t)c->E) return fail(BISIP_EHIP, "internal: tier %d has no image of this layout", tier);
        const double *src = &T.image[per * s];
        if (tier == 1) { std::memcpy(Rlo, src, tri * sizeof(float)); src += lo_floats / 2; }
        std::memcpy(R, src, tri * sizeof(double)); src += tri;
        std::memcpy(bhat, src, n * sizeof(double)); src += n;
        std::memcpy(e, src, n * sizeof(double)); src += n;
        std::memcpy(elo, src, n * sizeof(double)); src += n;
        *rest = *src;
    } else {                                     // a lone spectrum's kernel arguments (host.h: fill_reduced)
        if (T.Rpacked.size() != tri || (tier == 1 && T.Rlo_packed.size() < tri) || T.bhat.size() != (size_t)n ||
            T.evec.size() != (size_t)n || T.elo.size() != (size_t)n)
            return fail(BISIP_EHIP, "internal: tier %d has no operands", tier);
        if (tier == 1) std::memcpy(Rlo, T.Rlo_packed.data(), tri * sizeof(float));
        std::memcpy(R, T.Rpacked.data(), tri * sizeof(double));
        std::memcpy(bhat, T.bhat.data(), n * sizeof(double));
        std::memcpy(e, T.evec.data(), n * sizeof(double));
        std::memcpy(elo, T.elo.data(), n * sizeof(double));
        *rest = T.rest;
    }
    *lconst = c->E > 1 ? c->reduced[s].lconst : c->lconst;
    const int v = effective_variant(c);
    if (v == BISIP_VARIANT_REDUCED) *runs = tier == 0;
    else if (v == BISIP_VARIANT_REDUCED_COMP) *runs = c->mixed ? c->tier_of[s] == tier : tier == 1;
    else *runs = 0;
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
    double Rfull[MAXN * MAXN] = {};              // the (n,n) layout chi2_kernel reads
    float Rlo_full[MAXN * MAXN] = {};
    for (int i = 0, k = 0; i < n; ++i)
        for (int j = i; j < n; ++j, ++k) {
            Rfull[i * n + j] = R[k];
            if (comp) Rlo_full[i * n + j] = Rlo[k];
        }
    for (int64_t w = 0; w < W; ++w) {
        const double *th = theta + w * n;
        bool inside = true;                      // kernels.h: in_prior -- strict, NaN -> false
        for (int q = 0; q < n; ++q) inside = inside && (lo[q] < th[q]) && (th[q] < hi[q]);
        const double chi2 = reduced_chi2_kernel(n, Rfull, comp ? Rlo_full : nullptr, bhat, e, elo, rest, th, comp != 0);
        out[w] = inside ? std::fma(-0.5, chi2, lconst) : -INFINITY;
    }
    return BISIP_OK;
}
