"""Plots of the shape of a posterior: histograms of every parameter and a corner plot.

The reference draws these with ``ax.hist`` (src/bisip/plotlib.py:56-90) and the ``corner`` package
(src/bisip/plotlib.py:233-259) from a copy of the chain.  Here both are drawn from counts --
``get_param_histogram`` / ``get_corner_histograms`` -- so a chain kept on the GPU (``fit(chain='device')``) is
counted there and only the counts reach matplotlib, which is imported when a plot is asked for.
"""

import numpy as np


class plotlib(object):
    """Mixin with the histogram plots (mixed into Inversion)."""

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
