"""The row-list primitives of the lock-step executor (a control-flow path's particles as ascending int64 indices):
pp_partition_rows (a branch), pp_logweight_accumulate_rows (an observe / prior term on a path), pp_copy_rows (a path's result)
against their torch formulations, and the executor with PP_IS_ROWS=1 against the boolean-mask bookkeeping (PP_IS_ROWS=0).
Reference semantics: one trace at a time takes its own branches (pyprob/model.py:59-68); state.py:147-149, 211-217."""
import os
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')
REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope='module')
def runner():
    from pyprob_amd.engine import ICEngine
    from pyprob_amd.is_engine import ISRunner
    from pyprob_amd.spec import NetSpec
    spec = NetSpec({'obs0': {'dim': 32}, 'obs1': {'dim': 32}}, lstm_dim=64)
    spec.add_address('mu', 'Normal')
    return ISRunner(ICEngine(spec, device='cuda:0', seed=3))


@pytest.mark.parametrize('poll', ['1', '0'], ids=['polled', 'copied'])
@pytest.mark.parametrize('n,frac', [(1, 1.0), (7, 0.5), (1024, 0.3), (1025, 0.0), (4097, 1.0), (200003, 0.215), (1000001, 0.5)])
def test_partition_rows_is_the_stable_split(runner, n, frac, poll, monkeypatch):
    # poll: the counts come back through pinned host memory the kernel writes in place (pp_partition_rows_polled, the default)
    # or through an 8-byte device-to-host copy (pp_partition_rows)
    monkeypatch.setenv('PP_IS_PART_POLL', poll)
    g = torch.Generator(device='cpu').manual_seed(n)
    cond = (torch.rand(n, generator=g) < frac).cuda()
    t, f, nt, nf = runner.partition(cond, None, n)
    assert (nt, nf) == (int(cond.sum()), n - int(cond.sum()))
    assert torch.equal(t, torch.nonzero(cond).reshape(-1)) and torch.equal(f, torch.nonzero(~cond).reshape(-1))
    # a path's rows: every third particle, split again by the condition
    rows = torch.arange(0, n, 3, device='cuda')
    t, f, nt, nf = runner.partition(cond, rows, int(rows.numel()))
    assert torch.equal(t, rows[cond[rows]]) and torch.equal(f, rows[~cond[rows]])
    assert nt == int(t.numel()) and nf == int(f.numel()) and nt + nf == int(rows.numel())
    # several partitions in flight before the first is read (nested paths of the executor): one slot each
    handles = [runner.partition_launch(cond, None, n) for _ in range(5)]
    for h in reversed(handles):
        assert runner.partition_read(h)[2:] == (int(cond.sum()), n - int(cond.sum()))


class _Dist:
    """The duck type DistRunner.dist_term reads (pyprob/distributions/*.py attribute names)."""
    def __init__(self, name, **kw):
        self.name = name
        self.__dict__.update(kw)


def test_accumulate_rows_and_copy_rows(runner):
    from pyprob_amd.is_engine import DistTerm, MixTerm, ScalarTerm
    import mixture_cases as MC
    n = 50001
    g = torch.Generator(device='cpu').manual_seed(5)
    x = torch.randn(n, generator=g).cuda()
    mean = torch.randn(n, generator=g).cuda()
    sd = torch.tensor([1.7], device='cuda')
    rows = torch.nonzero(torch.rand(n, generator=g) < 0.2).reshape(-1).cuda()
    mask = torch.zeros(n, dtype=torch.bool, device='cuda').index_fill_(0, rows, True)
    term = runner.dist_term(_Dist('Normal', mean=mean, stddev=sd))
    assert type(term) is ScalarTerm and term.kind == 0 and (term.s0, term.s1) == (1, 0)       # per-particle mean, shared stddev
    assert term.p0.data_ptr() == mean.data_ptr() and term.p1.data_ptr() == sd.data_ptr()
    for xx in (x, torch.tensor([0.3], device='cuda')):
        lw_a = torch.randn(n, generator=g).cuda()
        lw_b = lw_a.clone()
        runner.accumulate(lw_a, term, xx, 0.5, rows=rows)                   # the path kept as its row list
        runner.accumulate(lw_b, term, xx, 0.5, rows=rows, mask=mask)        # ... and as a mask
        assert torch.equal(lw_a[~mask], lw_b[~mask])
        torch.testing.assert_close(lw_a, lw_b, rtol=1e-6, atol=1e-6)
    with pytest.raises(RuntimeError):
        runner.accumulate(torch.zeros(n + 1, device='cuda'), term, x, 0.5, rows=rows)       # (the mean holds n values)
    dst = torch.zeros(n, device='cuda')
    runner.copy_rows(x, dst, rows)
    assert torch.equal(dst, torch.where(mask, x, torch.zeros_like(x)))
    runner.copy_rows(torch.tensor([2.5], device='cuda'), dst, rows[:10])
    assert torch.equal(dst[rows[:10]], torch.full((10,), 2.5, device='cuda')) and torch.equal(dst[rows[10:]], x[rows[10:]])

    # One term of each type (and a Categorical, whose parameter is a row per particle) at n = 1000 - three full 256-lane workgroups and a partial one - on 257 rows (a second workgroup of
    # one lane) that include the first and the last particle: rows against mask as above, and rows, mask and full width against
    # the float64 log-density at the 1e-4 relative bar of tests/test_gpu_logweight.py (atol 1e-5: its bar for a log-density; one
    # fp32 rounding of lw + 0.5 lp at |lw| < 10 is 1e-6).
    n = 1000
    u, z = (lambda: torch.rand(n, generator=g)), (lambda: torch.randn(n, generator=g))
    rows = torch.cat([torch.tensor([0, n - 1]), torch.randperm(n - 2, generator=g)[:255] + 1]).sort().values.cuda()
    assert rows.numel() == 257 and int(rows[0]) == 0 and int(rows[-1]) == n - 1
    mask = torch.zeros(n, dtype=torch.bool, device='cuda').index_fill_(0, rows, True)
    m, conc, mm, w = z(), 1.0 + 2.0 * u(), z(), 0.1 + torch.rand(n, 3, generator=g)
    xn, xg, xm = z(), 0.1 + 3.0 * u(), 1.5 * u()
    pc, xc = 0.1 + torch.rand(n, 5, generator=g), torch.floor(5.0 * u())       # Categorical: one row of 5 weights per particle
    lpc = np.log(pc.double().numpy()[np.arange(n), xc.long().numpy()] / pc.double().numpy().sum(1))
    c = lambda v: torch.as_tensor(v, dtype=torch.float32).reshape(-1).cuda()       # noqa: E731
    cases = [(ScalarTerm, _Dist('Normal', mean=m.cuda(), stddev=c(1.7)), xn, MC.comp_lp64('Normal', [m.numpy(), 1.7], xn.numpy())),
             (ScalarTerm, _Dist('Categorical', probs=pc.cuda(), num_categories=5), xc, lpc),
             (DistTerm, _Dist('Gamma', concentration=conc.cuda(), rate=c(1.5)), xg, MC.comp_lp64('Gamma', [conc.numpy(), 1.5], xg.numpy())),
             (MixTerm, _Dist('Mixture', probs=w.cuda(), distributions=[
                 _Dist('Normal', mean=mm.cuda(), stddev=c(1.0)),
                 _Dist('TruncatedNormal', mean_non_truncated=c(0.0), stddev_non_truncated=c(1.0), low=c(-1.0), high=c(2.0)),
                 _Dist('Exponential', rate=c(2.0))]), xm,
              MC.mix_lp64(['Normal', 'TruncatedNormal', 'Exponential'], [[mm.numpy(), 1.0], [0.0, 1.0, -1.0, 2.0], [2.0]], w.numpy(), xm.numpy()))]
    for kind, dist, xx, lp64 in cases:
        term = runner.dist_term(dist)
        assert type(term) is kind
        lw0 = z()
        lw_a, lw_b, lw_c = lw0.cuda(), lw0.cuda(), lw0.cuda()
        runner.accumulate(lw_a, term, xx.cuda(), 0.5, rows=rows)
        runner.accumulate(lw_b, term, xx.cuda(), 0.5, rows=rows, mask=mask)
        runner.accumulate(lw_c, term, xx.cuda(), 0.5)
        assert torch.equal(lw_a[~mask], lw0.cuda()[~mask]) and torch.equal(lw_b[~mask], lw0.cuda()[~mask])
        torch.testing.assert_close(lw_a, lw_b, rtol=1e-6, atol=1e-6)
        want = lw0.double().numpy() + 0.5 * lp64
        touched = mask.cpu().numpy()
        for got in (lw_a, lw_b):
            np.testing.assert_allclose(got.cpu().numpy()[touched], want[touched], rtol=1e-4, atol=1e-5, err_msg=dist.name)
        np.testing.assert_allclose(lw_c.cpu().numpy(), want, rtol=1e-4, atol=1e-5, err_msg=dist.name)


def test_row_list_executor_equals_the_mask_executor(monkeypatch):
    """The same network and seeds: identical paths, values and log-weights whichever way a path's particles are kept."""
    import warnings
    sys.path.insert(0, os.path.join(REPO, 'tests'))
    from models import GaussianWithUnknownMeanMarsagliaLockStep
    from pyprob_amd.state import InferenceEngine, InferenceNetwork
    model = GaussianWithUnknownMeanMarsagliaLockStep()
    torch.manual_seed(3)
    out = {}
    with warnings.catch_warnings():
        warnings.simplefilter('ignore')
        model.learn_inference_network(inference_network=InferenceNetwork.LSTM, num_traces=8192, batch_size=256, lstm_dim=512, seed=3,
                                      observe_embeddings={'obs0': {'dim': 32}, 'obs1': {'dim': 32}})
        for mode in ('1', '0'):
            monkeypatch.setenv('PP_IS_ROWS', mode)
            post = model.posterior_results(30011, InferenceEngine.IMPORTANCE_SAMPLING_WITH_INFERENCE_NETWORK,
                                           observe={'obs0': 8, 'obs1': 9}, lock_step=True, seed=23)
            out[mode] = dict(v=post._all_values.cpu().numpy(), lw=post._all_log_weights.cpu().numpy(), paths=post.num_paths,
                             mean=float(post.mean), ess=float(post.effective_sample_size))
    a, b = out['1'], out['0']
    assert a['paths'] == b['paths'] > 3
    np.testing.assert_allclose(a['v'], b['v'], rtol=1e-6, atol=1e-6)
    fin = np.isfinite(b['lw'])
    assert np.array_equal(fin, np.isfinite(a['lw']))
    np.testing.assert_allclose(a['lw'][fin], b['lw'][fin], rtol=1e-5, atol=1e-5)
    assert abs(a['mean'] - b['mean']) < 1e-4 and abs(a['ess'] - b['ess']) < 1e-3 * b['ess']
