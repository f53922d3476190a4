"""bisip_amd -- MI355X-native implementation of BISIP's ensemble-MCMC likelihood hot path.

Drop-in for the model-class surface of ``bisip`` (reference: src/bisip/__init__.py):

    from bisip_amd import PolynomialDecomposition, DataFiles
    model = PolynomialDecomposition(DataFiles()['SIP-K389175'], nwalkers=32, nsteps=1000)
    model.fit()
    chain = model.get_chain(discard=500, thin=2, flat=True)

The arithmetic (prior + forward model + Gaussian log-likelihood for every walker)
runs in hand-written gfx950 kernels behind the C ABI of ``include/bisip_hip.h``.
"""

from .autocorr import AutocorrError
from .batch import SpectraBatch
from .decomposition import DESCRIPTOR_NAMES, INTEGRATING_NAMES, integrating_params, rtd, rtd_descriptors
from .data import DataFiles
from .modes import MODE_NAMES, mode_descriptors, order_modes
from .models import (ColeCole, Dias2000, Inversion, PeltonColeCole, PolynomialDecomposition,
                     Shin2015)
from .sampler import DeviceEnsembleSampler, EnsembleSampler
from .utils import load_data, load_data_batch

__all__ = ('Inversion', 'PolynomialDecomposition', 'PeltonColeCole', 'ColeCole', 'Dias2000',
           'Shin2015', 'DataFiles', 'SpectraBatch', 'EnsembleSampler', 'DeviceEnsembleSampler',
           'load_data', 'load_data_batch', 'AutocorrError', 'INTEGRATING_NAMES', 'rtd', 'integrating_params',
           'rtd_descriptors', 'DESCRIPTOR_NAMES', 'MODE_NAMES', 'order_modes', 'mode_descriptors')
