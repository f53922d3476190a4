"""What the three fused passes over a device-resident chain (bisip_response_moments_dev, bisip_fit_quality_dev,
bisip_predictive_check_dev) refuse, and in which words: one table of broken argument lists, walked through all three
entry points, with the exception type and the whole message of each; and pairs of faults adjacent in the order of the
rules, of which the earlier one must be the one reported.  Every call is refused on the host before a launch and goes
through chain_harness.GuardedCall: a refused call that wrote an output, the workspace or a guard fails."""
import pytest

from chain_harness import INT_FILL, SENTINEL, WORK_FILL, GuardedCall
from test_gpu_fit_quality import chain_near_a_centre, context
from test_gpu_response import make_batch

pytestmark = pytest.mark.gpu

E, WP, N_FREQ, N_SHORT, N_LONG = 3, 3, 20, 4, 400          # 400 samples of 3 walkers: 1200 rows, two segments


class Entry:
    """One entry point: its outputs (name, shape, int64?), its words for "no output asked for", and how it is called."""

    def __init__(self, name, outputs, none_asked, extra=()):
        self.name, self.outputs, self.none_asked, self.extra = name, outputs, none_asked, extra

    def workspace(self, ctx, n, count=E):
        return getattr(ctx, self.name + '_workspace')(n, count, WP)

    def dev(self, ctx, a, ptrs, work):
        getattr(ctx, self.name + '_dev')(a['first'], a['count'], a['chain'], a['n'], a['stride'], WP, *self.extra, *ptrs, work,
                                         a['nbytes'], a['stream'])


ENTRIES = (
    Entry('response_moments', (('mean', (E, 2, N_FREQ), False), ('std', (E, 2, N_FREQ), False)),
          'neither mean nor std asked for', extra=('ri',)),
    Entry('fit_quality', tuple((k, (E, 2, N_FREQ), False) for k in ('mean_q', 'var_q', 'lmeh')),
          'neither mean_q nor var_q nor lmeh asked for'),
    Entry('predictive_check', (('pit', (E, 2, N_FREQ), False), ('row', (E, 3), False), ('sign_changes', (E, 2 * N_FREQ - 1), True)),
          'neither pit nor row nor sign_changes asked for'),
)


@pytest.fixture(scope='module')
def setup():
    import torch
    b = make_batch('PeltonColeCole', dict(n_modes=1), N_FREQ, WP, count=E)
    ctx = context(b, b.zn, b.zn_err)
    assert ctx.N == N_FREQ and ctx.ndim == 4
    chain = chain_near_a_centre(b, E, WP, N_LONG, seed=3)             # (400, 9, 4); the first 4 samples serve as n = 4
    yield ctx, torch.from_numpy(chain).cuda()
    ctx.close()
    b.close()


def refused(entry, ctx, tensor, message, sized_for=N_SHORT, asked=True, null_work=False, short=0, **broken):
    """One call of ``entry`` on a sound argument list of ``sized_for`` samples with ``broken`` laid over it: it must raise
    ValueError with exactly ``message`` (a callable: of the bytes of workspace the shape needs) and write nothing."""
    import torch
    need = entry.workspace(ctx, sized_for)
    assert need >= 0
    call = GuardedCall()
    ptrs = [call.out(name, shape, dtype=torch.int64 if integer else None, asked=asked) for name, shape, integer in entry.outputs]
    work = call.work(need)
    a = dict(first=0, count=E, chain=tensor.data_ptr(), n=sized_for, stride=E * WP * ctx.ndim, nbytes=need - short,
             stream=call.stream)
    a.update(broken)
    with pytest.raises(ValueError) as info:
        entry.dev(ctx, a, ptrs, 0 if null_work else work)
    assert str(info.value) == (message(need) if callable(message) else message), entry.name
    for (name, _, integer), got in zip(entry.outputs, call.finish()):
        assert (got == (INT_FILL if integer else SENTINEL)).all(), f'{entry.name}: the refused call wrote {name}'
    t, nbytes = call.workspace
    assert (t[:nbytes].cpu().numpy() == WORK_FILL).all(), f'{entry.name}: the refused call wrote the workspace'


SHAPE = 'bisip_hip: bad chain shape'
NULL = 'bisip_hip: null argument'
RANGE = 'bisip_hip: spectra [2, 4) of 3'
STRIDE = 'bisip_hip: sample_stride smaller than one sample'
ALIGNED = 'bisip_hip: buffers must be 8-byte aligned'


@pytest.mark.parametrize('entry', ENTRIES, ids=lambda e: e.name)
def test_one_fault(setup, entry):
    ctx, chain = setup
    ptr, row = chain.data_ptr(), E * WP * ctx.ndim
    assert entry.workspace(ctx, N_LONG) > 0                            # two segments: every entry needs a workspace
    assert entry.workspace(ctx, 0) < 0 and entry.workspace(ctx, N_SHORT, E + 1) < 0
    for message, kw in (
            (SHAPE, dict(n=0)),
            (SHAPE, dict(count=E + 1)),
            (NULL, dict(chain=0)),
            ('bisip_hip: ' + entry.none_asked, dict(asked=False)),
            (RANGE, dict(first=2, count=2)),
            (STRIDE, dict(stride=row - 1)),
            (ALIGNED, dict(chain=ptr + 4)),
            (lambda need: f'bisip_hip: workspace of {need - 1} bytes, need {need}', dict(sized_for=N_LONG, short=1)),
            (lambda need: f'bisip_hip: workspace of 0 bytes, need {need}', dict(sized_for=N_LONG, null_work=True))):
        refused(entry, ctx, chain, message, **kw)


@pytest.mark.parametrize('entry', ENTRIES, ids=lambda e: e.name)
def test_of_two_faults_the_earlier_rule_is_reported(setup, entry):
    """Pairs adjacent in the order shape, null chain, nothing asked for, spectrum range, stride, alignment, workspace."""
    ctx, chain = setup
    ptr, row = chain.data_ptr(), E * WP * ctx.ndim
    for message, kw in (
            (SHAPE, dict(n=0, chain=0)),
            (NULL, dict(chain=0, asked=False)),
            ('bisip_hip: ' + entry.none_asked, dict(asked=False, first=2, count=2)),
            (RANGE, dict(first=2, count=2, stride=2 * WP * ctx.ndim - 1)),
            (STRIDE, dict(stride=row - 1, chain=ptr + 4)),
            (ALIGNED, dict(chain=ptr + 4, sized_for=N_LONG, short=1))):
        refused(entry, ctx, chain, message, **kw)
