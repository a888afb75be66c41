"""GPU tests of the feature-table optimizers (csrc/svoxt_optim.hip) through FeatureSGD / FeatureRMSprop / FeatureAdam and
csrc.optim_step -> ctypes -> C ABI: the parameter and every state table against the numpy restatement
(tests/optim_restate.py) bit for bit, against torch.optim within the float32 bound of tests/test_optim_host.py, untouched
rows, the renderer's caches behind a step, state dicts to and from torch, rebind behind a prune, streams."""
import numpy as np
import pytest
import torch

import svox_t_amd as svox
import svox_t_amd.csrc as _C
from oracle import oracle as O
from tests import optim_restate as R
from tests import test_optim_host as H
from tests.util import Case

pytestmark = pytest.mark.gpu

MAKE = {"sgd": (svox.FeatureSGD, dict(lr=0.1)), "sgd_momentum": (svox.FeatureSGD, dict(lr=0.1, momentum=0.9)),
        "rmsprop": (svox.FeatureRMSprop, dict(lr=1e-2)), "adam": (svox.FeatureAdam, dict(lr=1e-2))}


def gradients(M, K, steps, seed):
    """`steps` float32 [M, K] gradients: ~40 % of the rows random (scales 1e-4 .. 1 per row), some rows zero but for one
    element in the LAST column, some rows all -0.0, the rest +0.0."""
    rng = np.random.default_rng(seed)
    scale = (10.0 ** rng.uniform(-4.0, 0.0, size=(M, 1))).astype(np.float32)
    out = []
    for _ in range(steps):
        u = rng.random(M)
        g = (rng.standard_normal((M, K)).astype(np.float32) * scale) * (u < 0.4)[:, None]
        last = (u >= 0.4) & (u < 0.5)
        g[last, K - 1] = rng.standard_normal(int(last.sum())).astype(np.float32)
        g[(u >= 0.5) & (u < 0.6)] = -0.0
        out.append(np.ascontiguousarray(g, np.float32))
    return out


def run_gpu(kind, lazy, p0, grads, gpu):
    cls, kw = MAKE[kind]
    p = torch.nn.Parameter(torch.from_numpy(p0).to(gpu))
    opt = cls([p], lazy=lazy, **kw)
    for g in grads:
        p.grad = torch.from_numpy(g).to(gpu)
        opt.step()
    st = opt.state[p]
    return p.detach().cpu().numpy(), {k: st[k].cpu().numpy() for k in R.STATE_KEYS[kind]}, opt, p


def run_restated(kind, lazy, p0, grads, t0=0, state=None):
    p, state = p0.copy(), dict(state or {})
    for t, g in enumerate(grads, t0 + 1):
        p, state = R.step(kind, p, g, state, t, lazy=lazy, **MAKE[kind][1])
    return p, state


def same_bits(a, b):
    return np.array_equal(R.bits(a), R.bits(b))


@pytest.mark.parametrize("lazy", [False, True], ids=["dense", "lazy"])
@pytest.mark.parametrize("K", [4, 28, 32, 31, 249])
@pytest.mark.parametrize("kind", list(MAKE))
def test_bits_equal_the_restatement(gpu, kind, K, lazy):
    M = 1003                                                 # the last wavefront (K = 249: the last block) is partial
    p0 = np.random.default_rng(K).standard_normal((M, K)).astype(np.float32)
    grads = gradients(M, K, 10, seed=K + 1)
    touched = R.touched_rows(grads[0])
    assert touched.any() and not touched.all() and (np.count_nonzero(grads[0], axis=1) == 1).any()
    want_p, want_s = run_restated(kind, lazy, p0, grads)
    got_p, got_s, _, _ = run_gpu(kind, lazy, p0, grads, gpu)
    assert same_bits(got_p, want_p), f"p: {(R.bits(got_p) != R.bits(want_p)).sum()} elements differ"
    assert set(got_s) == set(want_s) == set(R.STATE_KEYS[kind])
    for k in want_s:
        assert same_bits(got_s[k], want_s[k]), f"{k}: {(R.bits(got_s[k]) != R.bits(want_s[k])).sum()} elements differ"
    again_p, again_s, _, _ = run_gpu(kind, lazy, p0, grads, gpu)                 # the same inputs: the same bits
    assert same_bits(again_p, got_p) and all(same_bits(again_s[k], got_s[k]) for k in got_s)


def test_tables_that_are_not_16_byte_aligned_take_the_scalar_path(gpu):
    M, K = 203, 28
    rng = np.random.default_rng(5)
    host = [rng.standard_normal((M, K)).astype(np.float32) for _ in range(4)]
    host[1][rng.random(M) < 0.5] = 0
    host[3] = np.abs(host[3])
    flat = [torch.zeros(M * K + 4, device=gpu) for _ in range(4)]
    views = [f[1:1 + M * K].view(M, K) for f in flat]
    for v, h in zip(views, host):
        v.copy_(torch.from_numpy(h))
    assert all(v.data_ptr() % 16 == 4 and v.is_contiguous() for v in views)
    opt = svox.FeatureAdam([torch.nn.Parameter(torch.zeros(1, 1, device=gpu))], lr=1e-2)
    _C.optim_step("adam", views[0], views[1], views[2], views[3], opt._hyper(opt.param_groups[0], 7), True)
    want = R.adam(host[0], host[1], host[2], host[3], 7, 1e-2, lazy=True)
    for v, w, f in zip((views[0], views[2], views[3]), want, (flat[0], flat[2], flat[3])):
        assert same_bits(v.cpu().numpy(), w)
        assert float(f[0]) == 0 and not f[1 + M * K:].any()                       # nothing written outside the table


@pytest.mark.parametrize("lazy", [False, True], ids=["dense", "lazy"])
def test_adam_against_torch_on_the_gpu(gpu, lazy):
    """The bound of tests/test_optim_host.py with every optimizer on the GPU: truth is torch.optim.Adam in float64; the
    kernel's max |deviation| must be within 2x that of torch.optim.Adam in float32."""
    p0, grads = H.torch_inputs()
    truth_p, truth_s = H.run_torch("adam", torch.float64, lazy, p0, grads, device=gpu)
    t32_p, t32_s = H.run_torch("adam", torch.float32, lazy, p0, grads, device=gpu)
    got_p, got_s, _, _ = run_gpu("adam", lazy, p0, grads, gpu)
    ours, theirs = H.deviations(got_p, got_s, truth_p, truth_s), H.deviations(t32_p, t32_s, truth_p, truth_s)
    for key in ours:
        print(f"adam {'lazy' if lazy else 'dense'} {key}: kernel {ours[key]:.3e}  torch float32 {theirs[key]:.3e}  "
              f"ratio {ours[key] / max(theirs[key], 1e-300):.3f}")
    for key in ours:
        assert ours[key] <= 2.0 * theirs[key], (key, ours[key], theirs[key])


@pytest.mark.parametrize("K", [28, 31, 249])
@pytest.mark.parametrize("kind", ["sgd_momentum", "rmsprop", "adam"])
def test_untouched_rows_keep_their_bits_and_are_not_read(gpu, kind, K):
    """Canaries: every untouched row of p and of the state holds NaNs with the row's number as payload.  They survive,
    and no touched row turns NaN: the untouched rows were neither written nor read into a result."""
    M = 517
    rng = np.random.default_rng(K)
    g = rng.standard_normal((M, K)).astype(np.float32)
    keep = rng.random(M) < 0.6
    g[keep] = 0
    g[keep & (np.arange(M) % 2 == 0)] = -0.0
    canary = (np.uint32(0x7FC00000) | (np.arange(M, dtype=np.uint32)[:, None] * np.uint32(256) + np.arange(K, dtype=np.uint32) % 256))
    tabs = []
    for i in range(3):
        t = np.abs(rng.standard_normal((M, K)).astype(np.float32))
        t.view(np.uint32)[keep] = canary[keep] + np.uint32(i << 20)
        tabs.append(t)
    dev = [torch.from_numpy(t).to(gpu) for t in tabs]
    ns = _C.OPTIM_STATES[kind]
    opt = MAKE[kind][0]([torch.nn.Parameter(torch.zeros(1, 1, device=gpu))], **MAKE[kind][1])
    _C.optim_step(kind, dev[0], torch.from_numpy(g).to(gpu), dev[1], dev[2] if ns == 2 else None,
                  opt._hyper(opt.param_groups[0], 3), True)
    for before, after in zip(tabs[:1 + ns], dev[:1 + ns]):
        after = after.cpu().numpy()
        assert same_bits(after[keep], before[keep])
        assert not np.isnan(after[~keep]).any() and not same_bits(after[~keep], before[~keep])
    if ns < 2:
        assert same_bits(dev[2].cpu().numpy(), tabs[2])


@pytest.mark.parametrize("static", [True, False], ids=["static_features", "default"])
def test_the_renderer_sees_the_updated_table(gpu, static):
    """forward + backward, FeatureAdam.step(), forward: the second image is the CPU oracle's render of the
    restatement-updated table, bit for bit -- the step moved the version counter, so no sigma mask or padded copy of the
    old table is reused."""
    c = Case(depth=5, K=28, data_format="SH9", width=64, height=64)
    tree = c.tree(gpu)
    if static:
        tree.static_features = True
    r = svox.VolumeRenderer(tree)
    rays = c.rays_gpu(gpu)
    opt = svox.FeatureAdam([tree.features], lr=1e-2)
    out = r(tree.features, rays, image_shape=(64, 64))
    first = out.detach().cpu().numpy()
    out.backward(svox.synth.grad_output(c.Q, out.shape[1]).to(gpu))
    version = tree.features._version
    grad = tree.features.grad.cpu().numpy()
    opt.step()
    assert tree.features._version > version
    with torch.no_grad():
        second = r(tree.features, rays, image_shape=(64, 64)).cpu().numpy()
    touched = R.touched_rows(grad)
    assert touched.any() and not touched.all()
    table, m, v = R.adam(c.features.numpy(), grad, np.zeros_like(grad), np.zeros_like(grad), 1, 1e-2, lazy=True)
    assert same_bits(tree.features.detach().cpu().numpy(), table)
    t = c.tree()
    ot = O.Tree(table, c.st.data, c.st.child, offset=t.offset.numpy(), scaling=t.invradius.numpy())
    want = O.volume_render(ot, *c.rays_np(), c.oracle_opts())
    assert not np.array_equal(first, second)
    np.testing.assert_array_equal(second, want)


def test_state_dict_round_trip_through_torch_adam(gpu):
    M, K = 300, 28
    p0 = np.random.default_rng(1).standard_normal((M, K)).astype(np.float32)
    grads = gradients(M, K, 4, seed=2)
    straight_p, straight_s, _, _ = run_gpu("adam", True, p0, grads, gpu)
    _, _, opt, p = run_gpu("adam", True, p0, grads[:3], gpu)
    theirs = torch.optim.Adam([p], lr=1e-2)
    theirs.load_state_dict(opt.state_dict())
    assert float(theirs.state[p]["step"]) == 3.0
    back = svox.FeatureAdam([p], lr=1e-2)
    back.load_state_dict(theirs.state_dict())
    p.grad = torch.from_numpy(grads[3]).to(gpu)
    back.step()
    assert float(back.state[p]["step"]) == 4.0
    assert same_bits(p.detach().cpu().numpy(), straight_p)
    for k in ("exp_avg", "exp_avg_sq"):
        assert same_bits(back.state[p][k].cpu().numpy(), straight_s[k])


@pytest.mark.parametrize("lazy", [False, True], ids=["dense", "lazy"])
@pytest.mark.parametrize("kind", ["adam", "sgd_momentum", "rmsprop"])
def test_a_state_dict_born_in_torch_optim_loads_and_steps(gpu, kind, lazy):
    """Two steps of torch.optim's optimizer, its state dict (no `lazy` in its groups) into ours, one more step: the bits
    of the restatement applied to torch's parameter and state."""
    M, K = 300, 28
    p0 = np.random.default_rng(6).standard_normal((M, K)).astype(np.float32)
    grads = gradients(M, K, 3, seed=7)
    torch_cls, kw = H.CASES[kind]
    p = torch.nn.Parameter(torch.from_numpy(p0).to(gpu))
    theirs = torch_cls([p], **kw)
    for g in grads[:2]:
        p.grad = torch.from_numpy(g).to(gpu)
        theirs.step()
    saved = theirs.state_dict()
    assert "lazy" not in saved["param_groups"][0]
    start_p = p.detach().cpu().numpy().copy()
    start_s = {k: theirs.state[p][k].cpu().numpy().copy() for k in R.STATE_KEYS[kind]}
    ours = MAKE[kind][0]([p], lazy=lazy, **MAKE[kind][1])
    ours.load_state_dict(saved)
    assert ours.param_groups[0]["lazy"] is lazy
    p.grad = torch.from_numpy(grads[2]).to(gpu)
    ours.step()
    want_p, want_s = run_restated(kind, lazy, start_p, grads[2:], t0=2, state=start_s)
    assert same_bits(p.detach().cpu().numpy(), want_p)
    for k in R.STATE_KEYS[kind]:
        assert same_bits(ours.state[p][k].cpu().numpy(), want_s[k]), k
    if kind != "sgd_momentum":
        assert float(ours.state[p]["step"]) == 3.0


def test_rebind_after_prune(gpu):
    c = Case(depth=5, K=28, data_format="SH9", width=32, height=32)
    tree = c.tree(gpu)
    M, K = tree.features.shape
    opt = svox.FeatureAdam([tree.features], lr=1e-2)
    grads = gradients(M, K, 2, seed=3)
    for g in grads:
        tree.features.grad = torch.from_numpy(g).to(gpu)
        opt.step()
    want_p, want_s = run_restated("adam", True, c.features.numpy(), grads)
    old = tree.features
    keep = torch.from_numpy(np.random.default_rng(4).random(c.st.child.shape) < 0.5).to(gpu)
    res = tree.prune(keep)
    assert tree.features is not old and 0 < tree.features.shape[0] < M
    row_map = res.row_map.cpu().numpy()
    with pytest.raises(RuntimeError, match="row_map"):
        opt.rebind(old, tree.features, res.row_map[:-1])
    opt.rebind(old, tree.features, res.row_map)
    assert opt.param_groups[0]["params"][0] is tree.features and old not in opt.state
    st = opt.state[tree.features]
    assert float(st["step"]) == 2.0
    for k in ("exp_avg", "exp_avg_sq"):
        assert same_bits(st[k].cpu().numpy(), want_s[k][row_map])
    g3 = gradients(row_map.shape[0], K, 1, seed=5)
    tree.features.grad = torch.from_numpy(g3[0]).to(gpu)
    opt.step()
    p3, s3 = run_restated("adam", True, want_p[row_map], g3, t0=2, state={k: v[row_map] for k, v in want_s.items()})
    assert same_bits(tree.features.detach().cpu().numpy(), p3)
    for k in ("exp_avg", "exp_avg_sq"):
        assert same_bits(opt.state[tree.features][k].cpu().numpy(), s3[k])
    # without a row_map: fresh state, zeros and step 0
    fresh = torch.nn.Parameter(tree.features.detach().clone())
    opt.rebind(tree.features, fresh)
    assert fresh not in opt.state
    fresh.grad = torch.from_numpy(g3[0]).to(gpu)
    opt.step()
    p4, s4 = run_restated("adam", True, p3, g3)
    assert float(opt.state[fresh]["step"]) == 1.0 and same_bits(fresh.detach().cpu().numpy(), p4)
    assert same_bits(opt.state[fresh]["exp_avg"].cpu().numpy(), s4["exp_avg"])


def test_step_on_a_side_stream_follows_the_backward_on_it(gpu, monkeypatch):
    """The step is issued on torch's CURRENT stream: the handle the C entry receives is the side stream's (checked on
    the call itself, so nothing rests on a race showing), and the table is the restatement's."""
    from svox_t_amd.csrc import _extras
    streams, real_call = [], _extras._call

    def recording_call(name, *args):
        if name == "svoxt_optim_step":
            streams.append(args[-1].value or 0)
        return real_call(name, *args)

    monkeypatch.setattr(_extras, "_call", recording_call)
    c = Case(depth=6, K=28, data_format="SH9", width=128, height=128)
    tree = c.tree(gpu)
    r = svox.VolumeRenderer(tree)
    rays = c.rays_gpu(gpu)
    opt = svox.FeatureAdam([tree.features], lr=1e-2)
    torch.cuda.synchronize()
    s = torch.cuda.Stream(device=gpu)
    with torch.cuda.stream(s):
        out = r(tree.features, rays, image_shape=(128, 128))
        out.backward(svox.synth.grad_output(c.Q, out.shape[1]).to(gpu))
        opt.step()
    assert streams == [s.cuda_stream] and s.cuda_stream != torch.cuda.default_stream(gpu).cuda_stream
    s.synchronize()
    grad = tree.features.grad.cpu().numpy()
    table, _, _ = R.adam(c.features.numpy(), grad, np.zeros_like(grad), np.zeros_like(grad), 1, 1e-2, lazy=True)
    assert R.touched_rows(grad).any() and same_bits(tree.features.detach().cpu().numpy(), table)
