"""The modes of a PeltonColeCole chain put in order, and the per-mode descriptors of the ordered row.

A multi-mode Cole-Cole posterior is symmetric under exchange of its modes: with the same prior box for every mode a chain
mixes the K! labellings, and a mean, an interval or an evidence is then taken over a mixture of K! copies of the posterior.
Ordering the modes of every sample by one parameter group picks one labelling (an identifiability constraint); the summaries
of the ordered chain are those of one copy.  This docstring is the one place the definitions are stated; the NumPy functions
below, the row function csrc/mode_order.h (the kernel k_mode_order<K> of csrc/chain_modes.hip and the host entry point
bisip_mode_order_host both call it) and the tests follow it.

A row is ``theta = (r0, m_1..m_K, log_tau_1..log_tau_K, c_1..c_K)``, ``1 <= K <= BISIP_MAX_MODES`` (5), ``ndim = 1 + 3K``.

Ordering
--------
* ``by`` selects the key group: ``'log_tau'`` (default), ``'m'`` or ``'c'``; in the C ABI ``key_group`` 1, 0, 2.
* ``perm = np.argsort(key, kind='stable')``: ascending by IEEE ``<``; ``-0.0`` and ``+0.0`` tie; every NaN sorts after
  ``+inf``; NaNs tie among themselves; ties keep the original mode order.
* The ordered row ``theta'``: position ``j`` of each of the three groups holds the values of mode ``perm[j]`` -- a pure
  permutation, the bits are copied.  ``r0`` stays.
* ``moved = perm != identity`` (any position).

Descriptors
-----------
``1 + 2K`` values of the ORDERED row, named by ``MODE_NAMES(K)`` = ``m_total, log_tau_cc1..K, log_tau_peak1..K``:

* ``m_total = (..((m'_1 + m'_2) + m'_3)..)``: plain additions in ascending ordered position.
* ``log_tau_cc_j = log_tau'_j + log1p(-m'_j) / c'_j``: the time constant of the Cole-Cole model in its conductivity form,
  ``tau_cc = tau (1 - m)^(1/c)`` (``1 / Z`` of one Pelton mode is ``(1 / r0) [1 + m / (1 - m) (1 - 1 / (1 + (i w tau_cc)^c))]``).
* ``log_tau_peak_j = log_tau'_j + log1p(-m'_j) / (2 c'_j)``: the relaxation time ``1 / omega`` at which the phase of mode ``j``
  taken alone peaks -- the geometric mean of ``tau`` and ``tau_cc``.
* Division is IEEE: a row at or beyond the box edge (``m = 1``, ``c = 0``) gives what IEEE gives, ``-inf`` or NaN, and the
  summaries of a chain that holds one propagate it as NumPy's do.

``log_tau`` is the natural logarithm, as in the model.

Exchangeability
---------------
For ``K >= 2`` ordering requires the bounds of ``m_j``, of ``log_tau_j`` and of ``c_j`` to be equal across ``j``: otherwise the
ordered region is not a fundamental domain of the prior and the methods raise a ValueError naming the first parameter that
differs.  ``K = 1`` orders nothing; the descriptors still apply.

* ``order_modes``, ``mode_permutation``, ``modes_moved``, ``mode_descriptors``: the definitions in NumPy;
* ``device_mode_order`` runs bisip_mode_order_dev on a ChainView (bisip_amd.chainview): the ordered rows and the descriptors
  are derived chains that the moments, percentiles and HDI summarise where they lie; ``host_mode_order`` goes through
  bisip_mode_order_host (no GPU);
* ``ModelModes`` and ``BatchModes`` are the methods of PeltonColeCole and of SpectraBatch.
"""

import math

import numpy as np

__all__ = ('KEY_GROUPS', 'MAX_MODES', 'MODE_NAMES', 'order_modes', 'mode_permutation', 'modes_moved', 'mode_descriptors',
           'check_exchangeable', 'log_symmetry', 'device_mode_order', 'host_mode_order', 'ModelModes', 'BatchModes')

KEY_GROUPS = {'m': 0, 'log_tau': 1, 'c': 2}      # key_group of bisip_mode_order_dev
MAX_MODES = 5                                    # include/bisip_hip.h: BISIP_MAX_MODES


def MODE_NAMES(n_modes):
    """The names of the outputs of ``mode_descriptors``: ``('m_total', 'log_tau_cc1', ..., 'log_tau_peak1', ...)``."""
    K = _mode_count(n_modes)
    return ('m_total',) + tuple(f'log_tau_cc{j + 1}' for j in range(K)) + tuple(f'log_tau_peak{j + 1}' for j in range(K))


def _mode_count(n_modes):
    K = int(n_modes)
    if not 1 <= K <= MAX_MODES:
        raise ValueError(f'n_modes={n_modes} out of range [1, {MAX_MODES}]')
    return K


def key_group(by):
    """``key_group`` of the C ABI for ``by``: 'm' 0, 'log_tau' 1, 'c' 2."""
    try:
        return KEY_GROUPS[by]
    except (KeyError, TypeError):
        raise ValueError(f"by must be 'log_tau', 'm' or 'c', got {by!r}") from None


def _rows(theta, n_modes):
    K = _mode_count(n_modes)
    theta = np.asarray(theta, dtype=np.float64)
    if theta.ndim < 1 or theta.shape[-1] != 1 + 3 * K:
        raise ValueError(f'theta must end in (r0, m_1..m_{K}, log_tau_1..{K}, c_1..{K}): {1 + 3 * K} values, got shape '
                         f'{theta.shape}')
    return theta, K


def mode_permutation(theta, n_modes, by='log_tau'):
    """``perm (..., K)``: position ``j`` of the ordered row takes mode ``perm[..., j]`` -- ``np.argsort(key, kind='stable')``."""
    theta, K = _rows(theta, n_modes)
    g = key_group(by)
    return np.argsort(theta[..., 1 + g * K:1 + (g + 1) * K], axis=-1, kind='stable')


def modes_moved(theta, n_modes, by='log_tau'):
    """``moved (...)``: True for the rows whose order differs from the stored one."""
    perm = mode_permutation(theta, n_modes, by)
    return np.any(perm != np.arange(perm.shape[-1]), axis=-1)


def order_modes(theta, n_modes, by='log_tau'):
    """Every row of ``theta (..., 1 + 3K)`` with its modes in ascending order of the key group ``by``: the same shape, the same
    bits in other places."""
    theta, K = _rows(theta, n_modes)
    perm = mode_permutation(theta, K, by)
    out = theta.copy()
    for g in range(3):
        out[..., 1 + g * K:1 + (g + 1) * K] = np.take_along_axis(theta[..., 1 + g * K:1 + (g + 1) * K], perm, axis=-1)
    return out


def mode_descriptors(theta, n_modes, by='log_tau'):
    """``(m_total, log_tau_cc_1..K, log_tau_peak_1..K)`` of every row of ``theta (..., 1 + 3K)`` after ordering by ``by``:
    ``(..., 1 + 2K)``, the module docstring's definition in NumPy."""
    o = order_modes(theta, n_modes, by)
    K = (o.shape[-1] - 1) // 3
    m, lt, c = o[..., 1:1 + K], o[..., 1 + K:1 + 2 * K], o[..., 1 + 2 * K:]
    out = np.empty(o.shape[:-1] + (1 + 2 * K,))
    with np.errstate(all='ignore'):
        total = m[..., 0].copy()
        for j in range(1, K):
            total = total + m[..., j]
        l = np.log1p(-m)
        out[..., 0] = total
        out[..., 1:1 + K] = lt + l / c
        out[..., 1 + K:] = lt + l / (2.0 * c)
    return out


def check_exchangeable(bounds, n_modes, names=None):
    """ValueError unless the bounds ``(2, 1 + 3K)`` of ``m_j``, of ``log_tau_j`` and of ``c_j`` are equal across ``j``; it names
    the first parameter whose bounds differ from those of mode 1.  ``K = 1`` passes."""
    K = _mode_count(n_modes)
    b = np.asarray(bounds, dtype=np.float64)
    if b.shape != (2, 1 + 3 * K):
        raise ValueError(f'bounds of shape {b.shape} for {K} modes: expected (2, {1 + 3 * K})')
    for g, group in enumerate(('m', 'log_tau', 'c')):
        for j in range(1, K):
            i = 1 + g * K + j
            if not np.array_equal(b[:, i], b[:, 1 + g * K]):
                name = names[i] if names is not None else f'{group}{j + 1}'
                raise ValueError(f'the modes are not exchangeable: the bounds of {name} {b[:, i].tolist()} differ from those of '
                                 f'mode 1 {b[:, 1 + g * K].tolist()}; ordering the modes needs the same box for every mode')


def log_symmetry(n_modes):
    """``log(K!)``: what the evidence over one labelling lacks of the evidence over the box."""
    return math.log(math.factorial(_mode_count(n_modes)))


# -- on the device and through the host entry point -------------------------------------------------------------------------
def device_mode_order(view, n_modes, by='log_tau', ordered=True, desc=True, moved=False):
    """bisip_mode_order_dev on the samples of a ChainView of ``ndim = 1 + 3K``: ``(ordered, desc, moved)``, new device tensors
    ``(n, n_ensembles * walkers_per_ensemble, 1 + 3K)`` and ``(..., 1 + 2K)`` float64 and ``(n, n_ensembles *
    walkers_per_ensemble)`` uint8, None for an output that is not asked for (it costs nothing).  ``view.derived`` of the first
    two is summarised as any chain is.  Asynchronous."""
    import torch
    from . import _hip
    K, g = _mode_count(n_modes), key_group(by)
    if view.ndim != 1 + 3 * K:
        raise ValueError(f'a chain of {view.ndim} parameters does not hold {K} Cole-Cole modes ({1 + 3 * K})')
    if not (ordered or desc or moved):
        raise ValueError('ask for one output at least')
    E, Wp = view.n_ensembles, view.walkers_per_ensemble
    o = view.empty((view.n, E * Wp, 1 + 3 * K), torch.float64) if ordered else None
    d = view.empty((view.n, E * Wp, 1 + 2 * K), torch.float64) if desc else None
    mv = view.empty((view.n, E * Wp), torch.uint8) if moved else None
    _hip.mode_order_dev(view.ptr, view.n, view.stride, E, Wp, K, g, *(0 if t is None else t.data_ptr() for t in (o, d, mv)),
                        view.stream)
    return o, d, mv


def host_mode_order(chain, n_modes, by='log_tau', n_ensembles=1, ordered=True, desc=True, moved=True):
    """The rows of ``device_mode_order`` by the same row function on the CPU (bisip_mode_order_host), no GPU: ``chain`` (n,
    rows, 1 + 3K) gives ``(ordered, desc, moved)`` as NumPy arrays (``moved`` bool), None where not asked for: ``ordered``,
    ``moved`` and ``m_total`` bit for bit what the kernel stores."""
    from . import _hip
    K, g = _mode_count(n_modes), key_group(by)
    chain = np.ascontiguousarray(chain, dtype=np.float64)
    if chain.ndim != 3 or chain.shape[2] != 1 + 3 * K:
        raise ValueError(f'the chain must be (n, rows, {1 + 3 * K}), got {chain.shape}')
    n, rows, ndim = chain.shape
    E = int(n_ensembles)
    if E < 1 or rows % E:
        raise ValueError(f'{rows} rows do not divide into {E} ensembles')
    return _hip.mode_order_host(chain, n, rows * ndim, E, rows // E, K, g, ordered, desc, moved)


def _order_argument(order_modes, n_modes, bounds, names=None):
    """``(K, by)`` for ``get_evidence(order_modes=by)`` after the exchangeability check; None for None."""
    if order_modes is None:
        return None
    key_group(order_modes)
    check_exchangeable(bounds, n_modes, names)
    return int(n_modes), order_modes


# -- the methods of PeltonColeCole and of SpectraBatch ------------------------------------------------------------------------
class ModelModes:
    """Mixin of PeltonColeCole (``_decomposition_samples`` is its ChainView of the samples to summarise, ``n_modes`` its mode
    count): the ordered posterior and the per-mode descriptors, per sample.  ``chain`` / ``discard`` / ``thin`` / ``flat`` as
    the get_integrating_* methods of PolynomialDecomposition; ``by``: the key group.  ``get_ordered_*`` act on the ``ndim``
    ordered parameters, ``get_mode_*`` on the ``1 + 2K`` descriptors (``MODE_NAMES``)."""

    def _exchangeable(self):
        check_exchangeable(self.param_bounds, self.n_modes, self.param_names)

    def order_modes(self, theta, by='log_tau'):
        """theta ``(ndim,)`` or ``(n, ndim)`` with its modes in ascending order of ``by`` (host)."""
        self._exchangeable()
        return order_modes(theta, self.n_modes, by)

    def mode_descriptors(self, theta, by='log_tau'):
        """``(m_total, log_tau_cc..., log_tau_peak...)`` of theta after ordering (host, MODE_NAMES): ``(1 + 2K,)`` or ``(n, 1 +
        2K)``."""
        self._exchangeable()
        return mode_descriptors(theta, self.n_modes, by)

    def _mode_views(self, by, chain, kwargs, ordered=False, desc=False, moved=False):
        key_group(by)
        self._exchangeable()
        view = self._decomposition_samples(chain, kwargs)
        return view, device_mode_order(view, self.n_modes, by, ordered, desc, moved)

    def _ordered_view(self, by, chain, kwargs):
        view, out = self._mode_views(by, chain, kwargs, ordered=True)
        return view.derived(out[0])

    def _descriptor_view(self, by, chain, kwargs):
        view, out = self._mode_views(by, chain, kwargs, desc=True)
        return view.derived(out[1])

    @staticmethod
    def _chain_of(view, chain, kwargs):
        flat = bool(kwargs.get('flat', False)) or chain is not None
        out = view.tensor.cpu().numpy()
        return out.reshape(-1, out.shape[-1]) if flat else out

    def get_ordered_chain(self, chain=None, by='log_tau', **kwargs):
        """The chain with the modes of every sample in order, permuted on the GPU: ``(n', nwalkers, ndim)`` as get_chain;
        ``(n, ndim)`` with ``flat=True`` or for a ``chain`` array."""
        return self._chain_of(self._ordered_view(by, chain, kwargs), chain, kwargs)

    def get_ordered_mean(self, chain=None, by='log_tau', **kwargs):
        """Posterior mean of the ordered parameters: ``(ndim,)`` (kwargs as get_param_mean)."""
        from .chainview import device_moments
        return device_moments(self._ordered_view(by, chain, kwargs))[0][0]

    def get_ordered_std(self, chain=None, by='log_tau', **kwargs):
        """Posterior standard deviation of the ordered parameters: ``(ndim,)``."""
        from .chainview import device_moments
        return device_moments(self._ordered_view(by, chain, kwargs))[1][0]

    def get_ordered_percentile(self, p=[2.5, 50, 97.5], chain=None, by='log_tau', **kwargs):
        """Percentiles of the ordered parameters: ``(len(p), ndim)``, ``(ndim,)`` for a scalar ``p``."""
        from .chainview import device_percentiles
        from .utils import first_if_scalar
        return first_if_scalar(p, device_percentiles(self._ordered_view(by, chain, kwargs), p)[:, 0, :])

    def get_ordered_hdi(self, mass=0.95, chain=None, by='log_tau', **kwargs):
        """The highest-density interval of the ordered parameters: ``(2, ndim)``; ``(len(mass), 2, ndim)`` for a sequence."""
        from .interval import device_hdi
        return device_hdi(self._ordered_view(by, chain, kwargs), mass)[..., 0, :]

    def get_mode_chain(self, chain=None, by='log_tau', **kwargs):
        """The per-mode descriptors of every sample, computed on the GPU: ``(n', nwalkers, 1 + 2K)`` as get_chain; ``(n, 1 +
        2K)`` with ``flat=True`` or for a ``chain`` array."""
        return self._chain_of(self._descriptor_view(by, chain, kwargs), chain, kwargs)

    def get_mode_mean(self, chain=None, by='log_tau', **kwargs):
        """Posterior mean of the per-mode descriptors: ``(1 + 2K,)``."""
        from .chainview import device_moments
        return device_moments(self._descriptor_view(by, chain, kwargs))[0][0]

    def get_mode_std(self, chain=None, by='log_tau', **kwargs):
        """Posterior standard deviation of the per-mode descriptors: ``(1 + 2K,)``."""
        from .chainview import device_moments
        return device_moments(self._descriptor_view(by, chain, kwargs))[1][0]

    def get_mode_percentile(self, p=[2.5, 50, 97.5], chain=None, by='log_tau', **kwargs):
        """Percentiles of the per-mode descriptors: ``(len(p), 1 + 2K)``, ``(1 + 2K,)`` for a scalar ``p``."""
        from .chainview import device_percentiles
        from .utils import first_if_scalar
        return first_if_scalar(p, device_percentiles(self._descriptor_view(by, chain, kwargs), p)[:, 0, :])

    def get_mode_hdi(self, mass=0.95, chain=None, by='log_tau', **kwargs):
        """The highest-density interval of the per-mode descriptors: ``(2, 1 + 2K)``; ``(len(mass), 2, 1 + 2K)`` for a
        sequence."""
        from .interval import device_hdi
        return device_hdi(self._descriptor_view(by, chain, kwargs), mass)[..., 0, :]

    def get_mode_switch_rate(self, by='log_tau', chain=None, **kwargs):
        """The share of each walker's used samples whose modes are stored in another order than ``by``'s: ``(nwalkers,)``.
        0 or 1 throughout: the walkers keep one labelling; in between: they switch."""
        import torch
        view, out = self._mode_views(by, chain, kwargs, moved=True)
        rate = out[2].to(torch.float64).mean(dim=0)
        view.synchronize()
        return rate.cpu().numpy()


class BatchModes:
    """Mixin of SpectraBatch (``_fitted()`` is its sampler): the methods of ModelModes for every spectrum, with a leading ``E``
    axis, on the device for ``chain='device'`` and ``'host'`` alike; refused for another model than PeltonColeCole."""

    def _cole_cole(self):
        if self.model != 'PeltonColeCole':
            raise ValueError(f'the ordering of modes and the per-mode descriptors belong to PeltonColeCole, not {self.model}')
        check_exchangeable(self.param_bounds, self.n_modes, self.param_names)

    def _mode_theta(self, theta):
        self._cole_cole()
        theta = np.asarray(theta, dtype=np.float64)
        if theta.ndim != 3 or theta.shape[0] != self.n_spectra:
            raise ValueError(f'theta must have shape ({self.n_spectra}, n, {self.ndim})')
        return theta

    def order_modes(self, theta, by='log_tau'):
        """theta ``(E, n, ndim)`` with the modes of every row in ascending order of ``by`` (host)."""
        return order_modes(self._mode_theta(theta), self.n_modes, by)

    def mode_descriptors(self, theta, by='log_tau'):
        """``(m_total, log_tau_cc..., log_tau_peak...)`` of theta ``(E, n, ndim)`` after ordering (host): ``(E, n, 1 + 2K)``."""
        return mode_descriptors(self._mode_theta(theta), self.n_modes, by)

    def _mode_views(self, by, discard, thin, ordered=False, desc=False, moved=False):
        self._cole_cole()
        key_group(by)
        view = self._fitted().used_samples_dev(discard, thin)
        return view, device_mode_order(view, self.n_modes, by, ordered, desc, moved)

    def _ordered_view(self, by, discard, thin):
        view, out = self._mode_views(by, discard, thin, ordered=True)
        return view.derived(out[0])

    def _descriptor_view(self, by, discard, thin):
        view, out = self._mode_views(by, discard, thin, desc=True)
        return view.derived(out[1])

    def _chain_of(self, view, flat):
        d = view.tensor
        ch = d.cpu().numpy().reshape(-1, self.n_spectra, self.nwalkers, d.shape[-1])
        if flat:
            ch = ch.transpose(1, 0, 2, 3).reshape(self.n_spectra, -1, d.shape[-1])
        return ch

    def get_ordered_chain(self, discard=0, thin=1, flat=False, by='log_tau'):
        """The chain with the modes of every sample in order: ``(n', E, Wp, ndim)`` as get_chain, ``(E, n' * Wp, ndim)`` with
        ``flat``."""
        return self._chain_of(self._ordered_view(by, discard, thin), flat)

    def get_ordered_mean(self, discard=0, thin=1, by='log_tau'):
        """Posterior mean of the ordered parameters per spectrum, ``(E, ndim)``."""
        from .chainview import device_moments
        return device_moments(self._ordered_view(by, discard, thin))[0]

    def get_ordered_std(self, discard=0, thin=1, by='log_tau'):
        """Posterior standard deviation of the ordered parameters per spectrum, ``(E, ndim)``."""
        from .chainview import device_moments
        return device_moments(self._ordered_view(by, discard, thin))[1]

    def get_ordered_percentile(self, p=(2.5, 50, 97.5), discard=0, thin=1, by='log_tau'):
        """Percentiles of the ordered parameters per spectrum, ``(len(p), E, ndim)`` (``(E, ndim)`` for a scalar ``p``)."""
        from .chainview import device_percentiles
        from .utils import first_if_scalar
        return first_if_scalar(p, device_percentiles(self._ordered_view(by, discard, thin), p))

    def get_ordered_hdi(self, mass=0.95, discard=0, thin=1, by='log_tau'):
        """The highest-density interval of the ordered parameters per spectrum, ``(2, E, ndim)`` (``(len(mass), 2, E, ndim)``
        for a sequence of masses)."""
        from .interval import device_hdi
        return device_hdi(self._ordered_view(by, discard, thin), mass)

    def get_mode_chain(self, discard=0, thin=1, flat=False, by='log_tau'):
        """The per-mode descriptors of every sample of every spectrum: ``(n', E, Wp, 1 + 2K)``, ``(E, n' * Wp, 1 + 2K)`` with
        ``flat``."""
        return self._chain_of(self._descriptor_view(by, discard, thin), flat)

    def get_mode_mean(self, discard=0, thin=1, by='log_tau'):
        """Posterior mean of the per-mode descriptors per spectrum, ``(E, 1 + 2K)``."""
        from .chainview import device_moments
        return device_moments(self._descriptor_view(by, discard, thin))[0]

    def get_mode_std(self, discard=0, thin=1, by='log_tau'):
        """Posterior standard deviation of the per-mode descriptors per spectrum, ``(E, 1 + 2K)``."""
        from .chainview import device_moments
        return device_moments(self._descriptor_view(by, discard, thin))[1]

    def get_mode_percentile(self, p=(2.5, 50, 97.5), discard=0, thin=1, by='log_tau'):
        """Percentiles of the per-mode descriptors per spectrum, ``(len(p), E, 1 + 2K)`` (``(E, 1 + 2K)`` for a scalar ``p``)."""
        from .chainview import device_percentiles
        from .utils import first_if_scalar
        return first_if_scalar(p, device_percentiles(self._descriptor_view(by, discard, thin), p))

    def get_mode_hdi(self, mass=0.95, discard=0, thin=1, by='log_tau'):
        """The highest-density interval of the per-mode descriptors per spectrum, ``(2, E, 1 + 2K)`` (``(len(mass), 2, E, 1 +
        2K)`` for a sequence of masses)."""
        from .interval import device_hdi
        return device_hdi(self._descriptor_view(by, discard, thin), mass)

    def get_mode_switch_rate(self, by='log_tau', discard=0, thin=1):
        """The share of each walker's used samples whose modes are stored in another order than ``by``'s: ``(E, Wp)``."""
        import torch
        view, out = self._mode_views(by, discard, thin, moved=True)
        rate = out[2].to(torch.float64).mean(dim=0)
        view.synchronize()
        return rate.cpu().numpy().reshape(self.n_spectra, self.nwalkers)
