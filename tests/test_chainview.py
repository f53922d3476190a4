"""bisip_amd.chainview on the host: the discard / thin arithmetic against NumPy's slice, the checks a ChainView
makes before any device work, and the public surface of the summaries that take one."""

import inspect

import numpy as np
import pytest

from bisip_amd.batch import SpectraBatch
from bisip_amd.chainview import ChainView, used_range
from bisip_amd.models import PolynomialDecomposition
from bisip_amd.sampler import DeviceEnsembleSampler, _SamplerBase
from bisip_amd.summaries import DeviceChainSummaries
from bisip_amd.utils import utils


def test_used_range_is_the_slice_of_get_chain():
    kept = refused = 0
    for n_total in range(1, 13):
        for discard in range(0, 14):
            for thin in range(1, 6):
                first = discard + thin - 1
                n = len(np.arange(n_total)[first::thin])
                if n:
                    assert used_range(n_total, discard, thin) == (first, n)
                    kept += 1
                else:
                    with pytest.raises(ValueError, match=f'no samples left with discard={discard}, thin={thin} of '
                                                         f'{n_total} stored'):
                        used_range(n_total, discard, thin)
                    refused += 1
    assert kept and refused


@pytest.mark.parametrize('discard,thin', [(0, 0), (0, -1), (-1, 1)])
def test_used_range_refuses_what_is_no_slice(discard, thin):
    with pytest.raises(ValueError, match='no samples left'):
        used_range(12, discard, thin)


def test_chain_view_wants_a_float64_tensor_on_the_gpu():
    torch = pytest.importorskip('torch')
    with pytest.raises(TypeError, match='float64 tensor on the GPU'):
        ChainView(torch.zeros((4, 6, 3), dtype=torch.float64), 4, 2, 3, 3)
    with pytest.raises(TypeError, match='float64 tensor on the GPU'):
        ChainView(torch.zeros((4, 6, 3), dtype=torch.float32), 4, 2, 3, 3)
    with pytest.raises(TypeError, match='float64 tensor on the GPU'):
        ChainView(np.zeros((4, 6, 3)), 4, 2, 3, 3)


# str(inspect.signature(...)) of every public summary, as the callers of the package know them
SURFACE = {
    'DeviceEnsembleSampler': {
        'device_chain': '(self)',
        'used_samples_dev': '(self, discard=0, thin=1, upload=True)',
        'param_moments': '(self, discard=0, thin=1)',
        'param_percentiles': '(self, p=(2.5, 50, 97.5), discard=0, thin=1)',
        'get_autocorr_time': '(self, discard=0, thin=1, c=5, tol=50, quiet=False)',
        'param_range': '(self, discard=0, thin=1)',
        'param_histograms': '(self, bins=25, range=None, discard=0, thin=1, bounds=None)',
        'pair_histograms': '(self, bins=20, range=None, discard=0, thin=1, bounds=None)',
        'trace_percentiles': '(self, p=(2.5, 50, 97.5), discard=0, thin=1)',
        'trace_mean': '(self, discard=0, thin=1)',
        'log_prob_samples_dev': '(self, discard=0, thin=1)',
        'log_prob_trace': '(self, p=(2.5, 50, 97.5), discard=0, thin=1)',
        'split_rhat': '(self, discard=0, thin=1, split=True)',
        'walker_moments': '(self, discard=0, thin=1)',
        'log_prob_rhat': '(self, discard=0, thin=1, split=True)',
        'integrating_chain_dev': '(self, log_tau, norm_factor, discard=0, thin=1)',
        'integrating_moments': '(self, log_tau, norm_factor, discard=0, thin=1)',
        'integrating_percentiles': '(self, p, log_tau, norm_factor, discard=0, thin=1)',
        'rtd_percentiles': '(self, p, log_tau, discard=0, thin=1)',
        'model_percentiles': '(self, p=(2.5, 50, 97.5), discard=0, thin=1)',
    },
    'SpectraBatch': {
        'get_param_mean': '(self, discard=0, thin=1)',
        'get_param_percentile': '(self, p=(2.5, 50, 97.5), discard=0, thin=1)',
        'get_model_percentile': '(self, p=(2.5, 50, 97.5), discard=0, thin=1)',
        'get_autocorr_time': '(self, discard=0, thin=1, c=5, tol=50, quiet=False)',
        'get_param_histogram': '(self, bins=25, range=None, discard=0, thin=1)',
        'get_corner_histograms': '(self, bins=20, range=None, discard=0, thin=1)',
        'get_trace_percentile': '(self, p=(2.5, 50, 97.5), discard=0, thin=1)',
        'get_trace_mean': '(self, discard=0, thin=1)',
        'get_log_prob_trace': '(self, p=(2.5, 50, 97.5), discard=0, thin=1)',
        'get_rhat': '(self, discard=0, thin=1, split=True)',
        'get_walker_mean': '(self, discard=0, thin=1)',
        'get_walker_std': '(self, discard=0, thin=1)',
        'get_log_prob_rhat': '(self, discard=0, thin=1, split=True)',
        'rtd': '(self, theta)',
        'integrating_params': '(self, theta)',
        'get_integrating_chain': '(self, discard=0, thin=1, flat=False)',
        'get_integrating_mean': '(self, discard=0, thin=1)',
        'get_integrating_std': '(self, discard=0, thin=1)',
        'get_integrating_percentile': '(self, p=(2.5, 50, 97.5), discard=0, thin=1)',
        'get_rtd_percentile': '(self, p=(2.5, 50, 97.5), discard=0, thin=1)',
        'get_param_std': '(self, discard=0, thin=1)',
        'get_chain': '(self, discard=0, thin=1, flat=False)',
        'get_log_prob': '(self, discard=0, thin=1)',
    },
    'utils': {
        'get_model_percentile': '(self, p=[2.5, 50, 97.5], chain=None, **kwargs)',
        'get_param_percentile': '(self, p=[2.5, 50, 97.5], chain=None, **kwargs)',
        'get_param_mean': '(self, chain=None, **kwargs)',
        'get_param_std': '(self, chain=None, **kwargs)',
        'get_param_histogram': '(self, bins=25, range=None, chain=None, **kwargs)',
        'get_corner_histograms': '(self, bins=20, range=None, chain=None, **kwargs)',
        'get_trace_percentile': '(self, p=[2.5, 50, 97.5], chain=None, **kwargs)',
        'get_trace_mean': '(self, chain=None, **kwargs)',
        'get_log_prob_trace': '(self, p=[2.5, 50, 97.5], **kwargs)',
        'get_rhat': '(self, chain=None, split=True, **kwargs)',
        'get_walker_mean': '(self, chain=None, **kwargs)',
        'get_walker_std': '(self, chain=None, **kwargs)',
        'get_log_prob_rhat': '(self, split=True, **kwargs)',
    },
    'PolynomialDecomposition': {
        'rtd': '(self, theta)',
        'integrating_params': '(self, theta)',
        'get_integrating_chain': '(self, chain=None, **kwargs)',
        'get_integrating_mean': '(self, chain=None, **kwargs)',
        'get_integrating_std': '(self, chain=None, **kwargs)',
        'get_integrating_percentile': '(self, p=[2.5, 50, 97.5], chain=None, **kwargs)',
        'get_rtd_percentile': '(self, p=[2.5, 50, 97.5], chain=None, **kwargs)',
    },
}


def test_public_surface_of_the_summaries_is_pinned():
    classes = {c.__name__: c for c in (DeviceEnsembleSampler, SpectraBatch, utils, PolynomialDecomposition)}
    got = {name: {m: str(inspect.signature(getattr(classes[name], m))) for m in methods}
           for name, methods in SURFACE.items()}
    assert got == SURFACE
    # the sampler's summaries are the mixin's own, its autocorrelation time included (not the host sampler's)
    assert set(SURFACE['DeviceEnsembleSampler']) <= set(vars(DeviceChainSummaries))
    assert DeviceEnsembleSampler.get_autocorr_time is not _SamplerBase.get_autocorr_time
    # nothing public of the other three is missing from the table
    for cls, more in ((SpectraBatch, {'rtd', 'integrating_params'}), (utils, set()),
                      (PolynomialDecomposition, {'rtd', 'integrating_params'})):
        assert {m for m in vars(cls) if m.startswith('get_')} | more == set(SURFACE[cls.__name__])
