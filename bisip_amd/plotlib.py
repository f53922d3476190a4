"""Plots of a chain: the walker traces, histograms of every parameter and a corner plot.

The reference draws these with ``ax.hist`` (src/bisip/plotlib.py:56-90) and the ``corner`` package
(src/bisip/plotlib.py:233-259) from a copy of the chain.  Here both are drawn from counts --
``get_param_histogram`` / ``get_corner_histograms`` -- so a chain kept on the GPU (``fit(chain='device')``) is
counted there and only the counts reach matplotlib, which is imported when a plot is asked for.

``plot_traces`` (src/bisip/plotlib.py:17-54) keeps the reference's figure.  One line per walker is what it draws from a
chain on the host with few walkers; a chain on the GPU, or a big ensemble, is drawn as a band of per-step percentiles
over the walkers (``get_trace_percentile``), so that again only the reduced numbers leave the device.
"""

import numpy as np

from .utils import discard_thin, refuse_discard_of_a_chain


class plotlib(object):
    """Mixin with the chain plots (mixed into Inversion)."""

    TRACE_LINES_MAX_WALKERS = 128      # style='auto': more walkers than this are drawn as a band

    def plot_traces(self, chain=None, p=(2.5, 50, 97.5), style='auto', **kwargs):
        """The traces of the MCMC simulation, one axis per parameter over the steps (src/bisip/plotlib.py:17-54).

        ``style='lines'``: one line per walker, ``ax.plot(chain[:, :, i], 'k', alpha=0.3)``, from ``chain (nsteps,
        nwalkers, ndim)`` or ``get_chain(**kwargs)`` -- the reference's picture.  ``style='band'``: the percentiles ``p``
        over the walkers at every step from ``get_trace_percentile`` -- the lowest to the highest filled, a line for
        each one in between (the median in ``'C3'``) -- against the index of the stored sample.  ``style='auto'``: lines
        for an explicit ``chain`` or a host sampler's chain of at most 128 walkers, else the band.  Returns the figure."""
        self._check_if_fitted()
        import matplotlib.pyplot as plt
        from . import trace as tr
        if style not in ('auto', 'lines', 'band'):
            raise ValueError(f"style={style!r}: 'auto', 'lines' or 'band'")
        if style == 'auto':
            if chain is not None:
                lines = np.ndim(chain) == 3
            else:
                on_host = not getattr(self._sampler, 'chain_on_device', False)
                lines = on_host and self.nwalkers <= self.TRACE_LINES_MAX_WALKERS
            style = 'lines' if lines else 'band'
        labels = self.param_names
        fig, axes = plt.subplots(self.param_bounds.shape[1], figsize=(8, 6), sharex=True, squeeze=False)
        axes = axes[:, 0]
        if style == 'lines':
            if chain is None:
                chain = self.get_chain(**kwargs)
            else:
                refuse_discard_of_a_chain(kwargs)
            chain = np.asarray(chain)
            if chain.ndim != 3:
                raise ValueError('A trace needs the unflattened chain (nsteps, nwalkers, ndim); do not pass flat=True.')
            for i, ax in enumerate(axes):
                ax.plot(chain[:, :, i], 'k', alpha=0.3)
            xlim = (0, len(chain))
        else:
            pp = np.sort(tr.check_percentiles(p))
            if pp.size < 1:
                raise ValueError('a band needs at least one percentile')
            pct = self.get_trace_percentile(pp, chain=chain, **kwargs)
            n = pct.shape[1]
            x = np.arange(n) if chain is not None else tr.used_steps(self._sampler.iteration, **discard_thin(kwargs))
            inner = range(1, pp.size - 1) if pp.size > 1 else range(1)
            for i, ax in enumerate(axes):
                if pp.size > 1:
                    ax.fill_between(x, pct[0, :, i], pct[-1, :, i], color='k', alpha=0.3, lw=0)
                for k in inner:
                    ax.plot(x, pct[k, :, i], c='C3' if pp[k] == 50 else 'k', lw=1)
            xlim = (x[0], x[-1] + 1) if chain is None else (0, n)
        for i, ax in enumerate(axes):
            ax.set_xlim(*xlim)
            ax.set_ylim(self.param_bounds[:, i])
            ax.set_ylabel(labels[i])
            ax.yaxis.set_label_coords(-0.1, 0.5)
        axes[-1].set_xlabel('Steps')
        fig.tight_layout()
        return fig

    def plot_histograms(self, chain=None, bins=25, **kwargs):
        """One histogram per parameter, ``bins`` equal bins between the smallest and largest sample, drawn with
        ``ax.stairs`` from ``get_param_histogram``.  ``chain`` or the ``discard`` / ``thin`` keywords as for
        ``get_chain`` (parse_chain).  Returns the figure."""
        self._check_if_fitted()
        import matplotlib.pyplot as plt
        counts, edges = self.get_param_histogram(bins=bins, chain=chain, **kwargs)
        labels = self.param_names
        ndim = counts.shape[0]
        fig, axes = plt.subplots(ndim, figsize=(5, 1.5 * ndim), squeeze=False)
        for i, ax in enumerate(axes[:, 0]):
            ax.stairs(counts[i], edges[i], fc='w', ec='k', fill=True)
            ax.set_xlabel(labels[i])
            ax.ticklabel_format(axis='x', scilimits=[-2, 2])
        fig.tight_layout()
        return fig

    def plot_corner(self, chain=None, bins=20, **kwargs):
        """Lower-triangle grid of the posterior: the histogram of parameter ``i`` on the diagonal (``ax.stairs``), the
        2-D counts of parameters ``(j, i)``, ``j < i``, below it (``ax.pcolormesh``, ``j`` along x), labelled with
        ``param_names``, from ``get_corner_histograms`` and ``get_param_histogram`` on the same edges.

        This is not the ``corner`` package: the counts are drawn as they are -- no smoothing, no contour levels, no
        quantile titles.  Returns the figure."""
        self._check_if_fitted()
        import matplotlib.pyplot as plt
        pair_counts, edges, (jj, kk) = self.get_corner_histograms(bins=bins, chain=chain, **kwargs)
        if chain is None:      # (the advice about discard / thin was given once above)
            import warnings
            with warnings.catch_warnings():
                warnings.simplefilter('ignore', UserWarning)
                counts, _ = self.get_param_histogram(bins=bins, range=edges[:, [0, -1]], chain=chain, **kwargs)
        else:
            counts, _ = self.get_param_histogram(bins=bins, range=edges[:, [0, -1]], chain=chain, **kwargs)
        labels = self.param_names
        ndim = edges.shape[0]
        fig, axes = plt.subplots(ndim, ndim, figsize=(1.6 * ndim + 1, 1.6 * ndim + 1), squeeze=False)
        for i in range(ndim):
            for j in range(ndim):
                ax = axes[i, j]
                if j > i:
                    ax.set_axis_off()
                    continue
                if j == i:
                    ax.stairs(counts[i], edges[i], color='k')
                    ax.set_yticks([])
                else:          # pair (j, i): first parameter j along x, second along y
                    q = int(np.flatnonzero((jj == j) & (kk == i))[0])
                    ax.pcolormesh(edges[j], edges[i], pair_counts[q].T, cmap='Greys')
                    ax.set_ylim(edges[i][0], edges[i][-1])
                ax.set_xlim(edges[j][0], edges[j][-1])
                if i == ndim - 1:
                    ax.set_xlabel(labels[j])
                else:
                    ax.set_xticklabels([])
                if j == 0 and i > 0:
                    ax.set_ylabel(labels[i])
                elif j != i or i == 0:
                    ax.set_yticklabels([])
        fig.tight_layout()
        return fig
