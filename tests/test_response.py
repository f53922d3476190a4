"""bisip_amd.response on the host: amplitude and minus phase against complex arithmetic on the golden forward outputs, the
NumPy restatement of the moments kernel's summation order against the long-double definitions within the bound of
tests/response_bounds.py, the plans, the new entry points and the surface of the models and of SpectraBatch."""
import inspect
import os
import re

import numpy as np
import pytest

from bisip_amd import response as rs
from conftest import case_id, case_model, golden_cases
from response_bounds import assert_within, reference_and_bounds, responses

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ordered_response_moments takes the PA representation with NumPy's hypot / arctan2 (glibc): each within 1 ulp of the
# exact value, and 1 ulp <= 2 u |x|, u = 2^-53: K = 2 in the term K u |x| of response_bounds
K_GLIBC = (2, 2)
ULP4 = 4 * 2.0 ** -52      # 4 ulp of the value: hypot / atan2 on one side, cabs / carg on the other, 1 ulp each


def one_case_per_model():
    seen, out = set(), []
    for path in golden_cases():
        if case_model(path) not in seen:
            seen.add(case_model(path))
            out.append(path)
    assert len(out) == 4
    return out


# -- the definitions ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('path', one_case_per_model(), ids=case_id)
def test_response_pa_against_complex_arithmetic(path):
    Z = np.load(path)['Z']                                   # (rows, 2, N): the reference's forward
    z = Z[:, 0, :] + 1j * Z[:, 1, :]
    pa = rs.response_pa(Z)
    assert pa.shape == Z.shape
    fin = np.isfinite(z)
    assert fin.any()
    amp, mph = np.abs(z), -np.angle(z)
    assert (np.abs(pa[:, 0][fin] - amp[fin]) <= ULP4 * amp[fin]).all()
    assert (np.abs(pa[:, 1][fin] - mph[fin]) <= ULP4 * np.abs(mph[fin])).all()
    assert (pa[:, 0][fin] >= 0).all() and (np.abs(pa[:, 1][fin]) <= np.pi).all()
    np.testing.assert_array_equal(rs.represent(Z, 'ri'), Z)
    np.testing.assert_array_equal(rs.represent(Z, 'pa'), pa)
    p = [2.5, 50, 97.5]
    np.testing.assert_array_equal(rs.model_percentile_pa(Z, p), np.percentile(pa, p, axis=0))
    for kind in rs.KINDS:
        mean, std = rs.response_moments(Z, kind)
        np.testing.assert_array_equal(mean, np.mean(rs.represent(Z, kind), axis=0))
        np.testing.assert_array_equal(std, np.std(rs.represent(Z, kind), axis=0))


@pytest.mark.parametrize('lead', [(), (0,), (1,), (2,), (3, 2)])
def test_response_pa_shapes(lead):
    Z = np.random.default_rng(len(lead)).normal(size=lead + (2, 5))
    pa = rs.response_pa(Z)
    assert pa.shape == lead + (2, 5) and pa.dtype == np.float64
    if Z.size:
        np.testing.assert_array_equal(pa[..., 0, :], np.hypot(Z[..., 0, :], Z[..., 1, :]))
        np.testing.assert_array_equal(pa[..., 1, :], -np.arctan2(Z[..., 1, :], Z[..., 0, :]))


def test_response_pa_sign_and_values():
    # a capacitive response (Im Z < 0) has a negative phase: minus the phase is positive, as -data['pha']
    pa = rs.response_pa(np.array([[3.0], [-4.0]]))
    assert pa[0, 0] == 5.0 and pa[1, 0] == np.arctan2(4.0, 3.0) > 0
    assert np.isnan(rs.response_pa(np.array([[np.nan], [1.0]]))).all()
    with pytest.raises(ValueError, match='2, N'):
        rs.response_pa(np.zeros((4, 3, 5)))
    with pytest.raises(ValueError, match="'ri' or 'pa'"):
        rs.represent(np.zeros((2, 3)), 'amp')
    with pytest.raises(ValueError, match="'ri' or 'pa'"):
        rs.response_moments(np.zeros((4, 2, 3)), 'xy')


# -- the device's order, restated -----------------------------------------------------------------------------------
# (E, rows, N): rows on both sides of a run of 64 slots and of the 256 slots, one row, one above the segment minimum (two
# segments, the second of one row), two ragged segments and a third; E = 256 is the first count that takes one segment
SHAPES = [(1, 1, 4), (1, 63, 4), (1, 64, 4), (1, 65, 4), (3, 65, 5), (1, 257, 3), (1, 1025, 3), (3, 1025, 2), (1, 2500, 2),
          (256, 65, 2), (256, 1, 1)]


@pytest.mark.parametrize('kind', rs.KINDS)
@pytest.mark.parametrize('shape', SHAPES, ids=lambda s: 'x'.join(map(str, s)))
def test_ordered_moments_against_the_definition(shape, kind):
    E, R, N = shape
    Z = responses(E, R, N)
    mean, std = rs.ordered_response_moments(Z, kind)
    assert mean.shape == std.shape == (E, 2, N)
    ref = reference_and_bounds(Z, kind, K_GLIBC)
    worst = max(assert_within(mean, ref, 'mean', str(shape)), assert_within(std, ref, 'std', str(shape)))
    print(f'{shape} {kind}: error at most {worst:.3f} of its bound')
    assert (std >= 0).all()
    if R > 1:
        with np.errstate(all='ignore'):
            rel = (ref['dstd'] / ref['std'])[:, 0, 1:]
        assert rel.max() < 1e-9                               # else the bound says nothing: the inputs would be wrong
        dm, ds = rs.response_moments(np.moveaxis(Z, 1, 0), kind)
        np.testing.assert_allclose(mean, dm, rtol=1e-12, atol=1e-300)
        np.testing.assert_allclose(std[:, :, 1:], ds[:, :, 1:], rtol=1e-7, atol=1e-300)
    if kind == 'ri':
        assert (std[E - 1, :, 0] == 0.0).all() and (mean[E - 1, :, 0] == Z[E - 1, 0, :, 0]).all()      # a constant: exact
    else:
        assert (std == 0.0).all() if R == 1 else True
    if E == 1:
        m3, s3 = rs.ordered_response_moments(Z[0], kind)       # (R, 2, N): one spectrum
        np.testing.assert_array_equal(m3, mean)
        np.testing.assert_array_equal(s3, std)


def test_ordered_moments_nan_stays_in_its_spectrum():
    Z = responses(3, 300, 4)
    Z[1, 17] = np.nan
    for kind in rs.KINDS:
        mean, std = rs.ordered_response_moments(Z, kind)
        assert np.isnan(mean[1]).all() and np.isnan(std[1]).all()
        assert np.isfinite(mean[[0, 2]]).all() and np.isfinite(std[[0, 2]]).all()


def test_plans():
    assert rs.plan(500, 512, 256) == (128000, 1, 256)                  # a survey: one segment per spectrum
    assert rs.plan(9, 256, 3) == (27, 1, 256) and rs.plan(9, 255, 3) == (1024, 1, 256)
    assert rs.plan(5000, 1, 32) == (1024, 157, 256)                    # the quickstart: cut to fill the chip
    assert rs.plan(600, 64, 64) == (1200, 32, 256)
    assert rs.plan(500, 3, 256) == (1024, 125, 256)
    for rows, nseg in ((1, 1), (63, 1), (64, 1), (65, 1), (1024, 1), (1025, 2), (2500, 3)):
        for E in (1, 3):
            assert rs.plan(rows, E, 1)[1:] == (nseg, 256) and rs.plan(1, E, rows)[1] == nseg
        assert rs.plan(rows, 256, 1) == (rows, 1, 256)
    with pytest.raises(ValueError):
        rs.plan(0, 1, 4)


# -- plumbing -------------------------------------------------------------------------------------------------------
NEW_ENTRIES = ('bisip_forward_columns_kind_dev', 'bisip_forward_percentiles_kind', 'bisip_response_moments_workspace',
               'bisip_response_moments_dev')


def test_entry_points_exist(hip_lib):
    import __graft_entry__ as entry
    from bisip_amd import _hip
    header = open(os.path.join(ROOT, 'include', 'bisip_hip.h')).read()
    for name in NEW_ENTRIES:
        assert hasattr(hip_lib, name) and name in _hip.SYMBOLS
        assert re.search(r'\b%s\(' % name, header)
    assert re.search(r'#define\s+BISIP_RESPONSE_RI\s+0\b', header) and re.search(r'#define\s+BISIP_RESPONSE_PA\s+1\b', header)
    assert _hip.RESPONSE_KINDS == {'ri': 0, 'pa': 1}
    assert hip_lib.bisip_abi_version() == entry.header_abi_version() == 6
    exports = open(os.path.join(ROOT, 'bisip_amd', 'csrc', 'exports.map')).read()
    assert 'bisip_*' in exports                                # every bisip_ symbol leaves the library
    for method in ('forward_percentiles_kind', 'forward_columns_kind_dev', 'response_moments_workspace',
                   'response_moments_dev'):
        assert callable(getattr(_hip.HipContext, method))
    with pytest.raises(ValueError, match="'ri' or 'pa'"):
        _hip.response_kind('phase')
    assert _hip.response_kind('pa') == 1 and _hip.response_kind(7) == 7


def test_signatures():
    import bisip_amd
    from bisip_amd.summaries import DeviceChainSummaries, device_model_percentiles
    sig = lambda f: str(inspect.signature(f))
    assert sig(DeviceChainSummaries.model_percentiles_pa) == '(self, p=(2.5, 50, 97.5), discard=0, thin=1)'
    assert sig(DeviceChainSummaries.model_moments) == "(self, kind='ri', discard=0, thin=1)"
    assert sig(device_model_percentiles) == "(view, ctx, p, kind='ri')"
    for cls in (bisip_amd.PolynomialDecomposition, bisip_amd.PeltonColeCole, bisip_amd.Dias2000, bisip_amd.Shin2015):
        assert sig(cls.get_model_percentile_pa) == '(self, p=[2.5, 50, 97.5], chain=None, **kwargs)'
        assert sig(cls.get_model_mean) == sig(cls.get_model_std) == "(self, chain=None, kind='ri', **kwargs)"
    B = bisip_amd.SpectraBatch
    assert sig(B.get_model_percentile_pa) == '(self, p=(2.5, 50, 97.5), discard=0, thin=1)'
    assert sig(B.get_model_mean) == sig(B.get_model_std) == "(self, kind='ri', discard=0, thin=1)"


def test_errors_of_an_unfitted_model_and_of_chain_with_discard():
    import bisip_amd
    path = bisip_amd.DataFiles()['SIP-K389175']
    m = bisip_amd.PeltonColeCole(path, n_modes=1, nwalkers=8, nsteps=5)
    for call in (m.get_model_percentile_pa, m.get_model_mean, m.get_model_std):
        with pytest.raises(AssertionError, match='not fitted'):
            call()
    chain = np.tile(0.5 * (m.param_bounds[0] + m.param_bounds[1]), (6, 1))
    for call in (m.get_model_percentile_pa, m.get_model_mean, m.get_model_std):
        with pytest.raises(ValueError, match='Do not pass both'):
            call(chain=chain, discard=2)
        with pytest.raises(ValueError, match='Flatten chain'):
            call(chain=chain.reshape(3, 2, -1))
    with pytest.raises(ValueError, match="'ri' or 'pa'"):
        m.get_model_mean(chain=chain, kind='amp')
    with pytest.raises(NotImplementedError, match='plotting'):
        m.plot_fit()
