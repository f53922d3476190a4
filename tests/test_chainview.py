"""bisip_amd.chainview on the host: the discard / thin arithmetic against NumPy's slice, and the checks a ChainView
makes before any device work."""

import numpy as np
import pytest

from bisip_amd.chainview import ChainView, used_range


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
