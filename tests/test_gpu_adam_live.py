"""pp_adam_step_live against pp_adam_step at the C ABI, bit for bit: a flat buffer of five tensors with 1, 3, 33, 2 and 40 chunks
(33 and 40 cross the 32-sub-counter boundary of the arrival tickets), random gradients, the dead tensors' gradients and moments
zero. Three consecutive steps through the live-chunk launch and through the full grid from identical state must leave the same
parameters, moments, cleared gradients, step counts and scratch words (all but PP_ADAM_SEEN: the full grid sets it per non-zero
gradient, the live launch per processed tensor), the arrival counters back at zero. The host side of the plan:
tests/test_adam_live_plan.py."""
import numpy as np
import pytest

from pyprob_amd import lib as L

pytestmark = pytest.mark.gpu
torch = pytest.importorskip('torch')

CHUNKS = (1, 3, 33, 2, 40)
NT = len(CHUNKS)
LR, B1, B2, EPS = 1e-3, 0.9, 0.999, 1e-8
TOP, FIRST_W, CHUNKS_W, SEEN = 1024, 1025, 1026, L.PP_ADAM_SEEN


def tensor_slice(t, chunks=CHUNKS):
    first = np.concatenate([[0], np.cumsum(chunks)])
    return slice(1024 * int(first[t]), 1024 * int(first[t + 1]))


class Flat:
    """One optimizer state on the device and the three ways to step it."""

    def __init__(self, dead=(), chunks=CHUNKS, seed=3, moments=(), bind=True):
        self.lib = L.load()
        self.dev = torch.device('cuda:0')
        self.chunks = chunks
        self.nt = len(chunks)
        self.first = np.ascontiguousarray(np.concatenate([[0], np.cumsum(chunks)]), np.int32)
        self.n = 1024 * int(self.first[-1])
        self.dead = tuple(dead)
        rng = np.random.default_rng(seed)
        self.P = torch.from_numpy(rng.standard_normal(self.n).astype(np.float32)).to(self.dev)
        m = np.zeros(self.n, np.float32)
        v = np.zeros(self.n, np.float32)
        for t in moments:          # a tensor whose moments the caller wrote (checkpoint load)
            s = tensor_slice(t, chunks)
            m[s] = (0.1 * rng.standard_normal(s.stop - s.start)).astype(np.float32)
            v[s] = (0.01 * rng.random(s.stop - s.start)).astype(np.float32)
        self.M, self.V = torch.from_numpy(m).to(self.dev), torch.from_numpy(v).to(self.dev)
        self.G = torch.zeros(self.n, device=self.dev)
        self.ct = torch.from_numpy(np.repeat(np.arange(self.nt), chunks).astype(np.int32)).to(self.dev)
        self.active = torch.ones(self.nt, device=self.dev)
        self.tstep = torch.zeros(self.nt, dtype=torch.int32, device=self.dev)
        self.scratch = torch.zeros(L.PP_ADAM_SCRATCH * self.nt, dtype=torch.int32, device=self.dev)
        if moments:                # what ICEngine.moments_written does for the full grid ...
            self.scratch.view(-1, L.PP_ADAM_SCRATCH)[:, SEEN] = 1
        self.skip = torch.zeros(1, dtype=torch.int32, device=self.dev)
        self.bound = False
        if bind:
            L.check(self.lib.pp_adam_live_bind(self.G.data_ptr(), self.M.data_ptr(), self.V.data_ptr(), self.n,
                                               self.first.ctypes.data, self.nt, 1), 'pp_adam_live_bind')
            self.bound = True
            for t in range(self.nt):   # ... and what the writers of the gradients do for the live launch
                if t not in self.dead:
                    s = tensor_slice(t, chunks)
                    self.lib.pp_adam_live_mark_range(self.G.data_ptr(), s.start, s.stop - s.start)

    def close(self):
        if self.bound:
            self.lib.pp_adam_live_unbind(self.G.data_ptr())
        self.bound = False

    def grads(self, k, zero=()):
        """Step k's gradients: random on the touched tensors, zero on the dead ones (and on `zero`)."""
        rng = np.random.default_rng(1000 + k)
        g = (0.1 * rng.standard_normal(self.n)).astype(np.float32)
        for t in tuple(self.dead) + tuple(zero):
            g[tensor_slice(t, self.chunks)] = 0.0
        return g

    def step(self, live, g, wd=0.0, zero_grads=True, gscale=1.0):
        self.G.copy_(torch.from_numpy(g))
        fn = self.lib.pp_adam_step_live if live else self.lib.pp_adam_step
        rc = fn(self.P.data_ptr(), self.G.data_ptr(), self.M.data_ptr(), self.V.data_ptr(), self.n, self.ct.data_ptr(),
                self.active.data_ptr(), self.tstep.data_ptr(), self.scratch.data_ptr(), self.nt, LR, B1, B2, EPS, wd, gscale,
                L.PP_ADAM_ZERO_GRADS if zero_grads else 0, self.skip.data_ptr(), None)
        L.check(rc, 'pp_adam_step')
        torch.cuda.synchronize()

    def snapshot(self):
        sc = self.scratch.cpu().numpy().reshape(self.nt, L.PP_ADAM_SCRATCH).copy()
        return dict(P=self.P.cpu().numpy(), M=self.M.cpu().numpy(), V=self.V.cpu().numpy(), G=self.G.cpu().numpy(),
                    step=self.tstep.cpu().numpy(), scratch=sc)


def assert_same(a, b, what):
    for k in ('P', 'M', 'V', 'G'):
        assert np.array_equal(a[k].view(np.uint32), b[k].view(np.uint32)), (what, k)
    assert np.array_equal(a['step'], b['step']), (what, a['step'], b['step'])
    keep = np.ones(L.PP_ADAM_SCRATCH, bool)
    keep[SEEN] = False
    assert np.array_equal(a['scratch'][:, keep], b['scratch'][:, keep]), what
    for s in (a, b):
        assert not s['scratch'][:, :TOP + 1].any(), what          # every arrival counter is back at zero
    assert np.array_equal(a['scratch'][:, [FIRST_W, CHUNKS_W]], b['scratch'][:, [FIRST_W, CHUNKS_W]]), what


def run(paths, dead=(), chunks=CHUNKS, inactive=(), skip_at=(), wd=0.0, zero_grads=True, zero=(), moments=(), gscale=1.0):
    """One state stepped len(paths) times, step k through the live launch where paths[k]; the snapshots after every step."""
    f = Flat(dead=dead, chunks=chunks, moments=moments)
    try:
        for t in inactive:
            f.active[t] = 0.0
        snaps = [f.snapshot()]
        for k, live in enumerate(paths):
            f.skip.fill_(1 if k in skip_at else 0)
            f.step(live, f.grads(k, zero=zero), wd=wd, zero_grads=zero_grads, gscale=gscale)
            snaps.append(f.snapshot())
        return snaps
    finally:
        f.close()


@pytest.fixture
def mode(monkeypatch):
    monkeypatch.setenv('PP_ADAM_LIVE', '1')
    return '1'


def both(**kw):
    full = run((False, False, False), **kw)
    live = run((True, True, True), **kw)
    for k in range(1, 4):
        assert_same(full[k], live[k], 'after step %d' % k)
    return full, live


@pytest.mark.parametrize('wt', ['1', '0'])
@pytest.mark.parametrize('dead', [(), (0,), (2,), (4,), (1, 2), (0, 2, 4)])
def test_dead_patterns(mode, monkeypatch, dead, wt):
    monkeypatch.setenv('PP_STORE_WT', wt)
    full, live = both(dead=dead)
    for t in range(NT):
        s = tensor_slice(t)
        assert live[3]['step'][t] == 3
        if t in dead:      # untouched: nothing but the step count moved
            assert np.array_equal(live[3]['P'][s].view(np.uint32), live[0]['P'][s].view(np.uint32))
            assert not live[3]['M'][s].any() and not live[3]['V'][s].any()
            assert live[3]['scratch'][t, SEEN] == 0
        else:
            assert not np.array_equal(live[3]['P'][s], live[0]['P'][s])
            assert live[3]['scratch'][t, SEEN] == 1
    assert not live[3]['G'].any()


def test_more_runs_than_the_table_holds(mode):
    both(dead=(1, 3, 5, 7), chunks=(2, 1, 34, 1, 2, 3, 1, 2, 1))      # five runs: the full grid, through the live entry


@pytest.mark.parametrize('dead', [(), (4,), (2, 4)])
def test_inactive_tensors_live_and_dead(mode, dead):
    full, live = both(dead=dead, inactive=(2, 4))
    assert live[3]['step'].tolist() == [3, 3, 0, 3, 0]
    s = tensor_slice(2)
    assert np.array_equal(live[3]['P'][s].view(np.uint32), live[0]['P'][s].view(np.uint32))
    if 2 not in dead:      # an inactive tensor's gradient is not consumed (and not cleared), as in the full grid
        assert live[3]['G'][s].any()


@pytest.mark.parametrize('zero_grads', [True, False])
def test_skip_flag(mode, zero_grads):
    full, live = both(dead=(3,), skip_at=(1,), zero_grads=zero_grads)
    assert live[3]['step'].tolist() == [2] * NT                    # the skipped call steps nothing, the dead tensor included
    for k in ('P', 'M', 'V'):
        assert np.array_equal(live[2][k].view(np.uint32), live[1][k].view(np.uint32))
    assert live[2]['G'].any() != zero_grads                        # the (non-finite) gradients are still cleared


def test_zero_grads_off(mode):
    full, live = both(dead=(2,), zero_grads=False)
    assert live[3]['G'].any()


def test_live_tensor_with_zero_gradient_and_zero_moments(mode):
    """Tensor 2 is in the live list but its gradient is zero every step: p - step_size * (0 / (0 + eps)) = p, m = v = 0."""
    full, live = both(zero=(2,))
    s = tensor_slice(2)
    assert np.array_equal(live[3]['P'][s].view(np.uint32), live[0]['P'][s].view(np.uint32))
    assert not live[3]['M'][s].any() and not live[3]['V'][s].any()
    assert live[3]['step'][2] == 3 and full[3]['step'][2] == 3
    assert live[3]['scratch'][2, SEEN] == 1 and full[3]['scratch'][2, SEEN] == 0     # the one word that may differ


def test_touched_tensor_with_moments_and_zero_gradient(mode):
    full, live = both(zero=(2,), moments=(0, 1, 2, 3, 4))
    s = tensor_slice(2)
    for k in range(1, 4):
        want = np.float32(B1) * live[k - 1]['M'][s]
        assert np.array_equal(live[k]['M'][s].view(np.uint32), want.view(np.uint32)), k
        assert not np.array_equal(live[k]['P'][s], live[k - 1]['P'][s])          # the old momentum still moves the weights


def test_weight_decay_updates_a_dead_tensor(mode):
    full, live = both(dead=(2, 4), wd=1e-2)
    for t in (2, 4):
        s = tensor_slice(t)
        assert not np.array_equal(live[1]['P'][s], live[0]['P'][s])
        assert live[3]['M'][s].any()


def test_grad_scale(mode):
    both(dead=(1,), gscale=0.25)


@pytest.mark.parametrize('paths', [(True, False, True), (False, True, False)])
def test_the_two_launches_alternate_on_one_state(mode, paths):
    """PP_ADAM_SEEN hand-over: the live launch sets the word for what it processed, so the full grid that follows does not take a
    (now non-zero) tensor for one whose moments are still zero - and the other way round."""
    full = run((False, False, False), dead=(2,))
    mixed = run(paths, dead=(2,))
    for k in range(1, 4):
        assert_same(full[k], mixed[k], 'after step %d' % k)
    # tensor 1 gets zero gradients after the first step: a full grid that trusted a stale PP_ADAM_SEEN = 0 would freeze its moments
    f = Flat(dead=(2,))
    try:
        f.step(paths[0], f.grads(0))
        g = f.grads(1, zero=(1,))
        f.step(paths[1], g)
        a = f.snapshot()
    finally:
        f.close()
    r = Flat(dead=(2,))
    try:
        r.step(False, r.grads(0))
        r.step(False, r.grads(1, zero=(1,)))
        b = r.snapshot()
    finally:
        r.close()
    assert_same(a, b, 'zero gradient after a non-zero one')
    s = tensor_slice(1)
    assert a['M'][s].any()


def test_switch_off_is_the_full_grid(monkeypatch):
    """PP_ADAM_LIVE=0: the live entry launches the full grid with the kernel pp_adam_step runs (PP_ADAM_SEEN included)."""
    monkeypatch.setenv('PP_ADAM_LIVE', '0')
    full = run((False, False, False), dead=(2,), zero=(1,))
    off = run((True, True, True), dead=(2,), zero=(1,))
    for k in range(1, 4):
        assert_same(full[k], off[k], k)
        assert np.array_equal(full[k]['scratch'], off[k]['scratch'])


def test_unbound_buffers_take_the_full_grid(mode):
    f = Flat(dead=(2,), bind=False)
    r = Flat(dead=(2,), bind=False)
    try:
        for k in range(2):
            f.step(True, f.grads(k))
            r.step(False, r.grads(k))
        a, b = f.snapshot(), r.snapshot()
        assert_same(a, b, 'unbound')
        assert np.array_equal(a['scratch'], b['scratch'])
    finally:
        f.close()
        r.close()
