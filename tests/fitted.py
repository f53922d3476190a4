"""The fitted models that the summary tests share: a PolynomialDecomposition whose chain comes from the host sampler
around a NumPy log-probability (nothing touches the device), and the one the device sampler fits.  Callers that want a
model once per session wrap these in functools.lru_cache themselves."""
import numpy as np

CENTRE = np.array([1.0, 0.01, 0.0, 0.0])


def gaussian_logp(theta):
    return -0.5 * np.sum((theta - CENTRE) ** 2 / 1e-4, axis=1)


def fitted_on_host(nsteps=20):
    import bisip_amd
    from bisip_amd.sampler import EnsembleSampler
    m = bisip_amd.PolynomialDecomposition(bisip_amd.DataFiles()['SIP-K389175'], poly_deg=2, nwalkers=8)
    np.random.seed(1)
    s = EnsembleSampler(8, 4, gaussian_logp)
    s.run_mcmc(CENTRE + 1e-3 * np.random.randn(8, 4), nsteps)
    m._sampler = s
    m._Inversion__fitted = True
    return m


def fitted_model(where='device', nsteps=120):
    import bisip_amd
    m = bisip_amd.PolynomialDecomposition(bisip_amd.DataFiles()['SIP-K389175'], poly_deg=2, nwalkers=32, nsteps=nsteps)
    np.random.seed(4)
    m.fit(chain=where)
    assert m._sampler.chain_on_device == (where == 'device')
    return m
