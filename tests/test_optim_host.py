"""The feature-table optimizers without a GPU: the numpy restatement of the kernel's arithmetic (tests/optim_restate.py)
on hand-made cases and against torch.optim, the C entry's and the operator's argument checks (all before any launch), the
Python surface and the bookkeeping of rebind.  The GPU half is tests/test_gpu_optim.py."""
import ctypes
import math

import numpy as np
import pytest
import torch

import svox_t_amd
import svox_t_amd.csrc as _C
from svox_t_amd import optim as FO
from svox_t_amd.csrc import _abi

from . import optim_restate as R

f32 = np.float32


def A(x):
    return np.array(x, np.float32)


# ----------------------------------------------------------------------------------------------------- hand-made cases
def test_sgd_by_hand():
    p, g = A([[1, 2], [3, 4]]), A([[0.5, -1], [0, 0]])
    for lazy in (True, False):                               # plain SGD: the same table in both modes
        assert np.array_equal(R.sgd(p, g, 0.5, lazy), A([[0.75, 2.5], [3, 4]]))


def test_momentum_first_step_and_untouched_row():
    p, g = A([[1, 2], [3, 4]]), A([[0.5, -1], [0, 0]])
    p1, b1 = R.sgd_momentum(p, g, np.zeros_like(p), 0.5, 0.5, lazy=True)
    assert np.array_equal(b1, g)                             # the buffer starts at zero: b = g on the first step
    assert np.array_equal(p1, A([[0.75, 2.5], [3, 4]]))
    g2 = A([[0, 0], [1, 1]])                                 # now row 0 is untouched
    p2, b2 = R.sgd_momentum(p1, g2, b1, 0.5, 0.5, lazy=True)
    assert np.array_equal(b2, A([[0.5, -1], [1, 1]])) and np.array_equal(p2, A([[0.75, 2.5], [2.5, 3.5]]))
    p2d, b2d = R.sgd_momentum(p1, g2, b1, 0.5, 0.5, lazy=False)         # dense: the buffer decays and still moves the row
    assert np.array_equal(b2d, A([[0.25, -0.5], [1, 1]])) and np.array_equal(p2d, A([[0.625, 2.75], [2.5, 3.5]]))


def test_rmsprop_by_hand():
    p, g = A([[1, 2], [3, 4]]), A([[2, -2], [0, 0]])
    v0 = A([[0, 0], [4, 4]])
    # v = 0.75 * 0 + 0.25 * 4 = 1; p -= 0.5 * (2 / (1 + 1))
    p1, v1 = R.rmsprop(p, g, v0, 0.5, alpha=0.75, eps=1.0, lazy=True)
    assert np.array_equal(v1, A([[1, 1], [4, 4]])) and np.array_equal(p1, A([[0.5, 2.5], [3, 4]]))
    p1d, v1d = R.rmsprop(p, g, v0, 0.5, alpha=0.75, eps=1.0, lazy=False)
    assert np.array_equal(v1d, A([[1, 1], [3, 3]])) and np.array_equal(p1d, p1)     # g = 0: v decays, p + (-lr)(0 / ..) = p


def test_adam_by_hand_untouched_row_keeps_bits_lazy_and_decays_dense():
    p, g = A([[1, 2], [3, 4]]), A([[3, -3], [0, 0]])
    m0, v0 = A([[0, 0], [1, 1]]), A([[0, 0], [4, 4]])
    kw = dict(t=1, lr=0.5, betas=(0.5, 0.75), eps=1.0)
    # row 0: m = 1.5, v = 0.25 * 9 = 2.25, d = 1.5 / sqrt(1 - 0.75) + 1 = 4, step = -0.5 / (1 - 0.5) = -1: p -= 0.375
    p1, m1, v1 = R.adam(p, g, m0, v0, lazy=True, **kw)
    assert np.array_equal(m1, A([[1.5, -1.5], [1, 1]])) and np.array_equal(v1, A([[2.25, 2.25], [4, 4]]))
    assert np.array_equal(p1, A([[0.625, 2.375], [3, 4]]))
    assert np.array_equal(R.bits(p1[1]), R.bits(p[1]))
    # dense: the moments of the row with g = 0 decay and the row moves along the old momentum
    pd, md, vd = R.adam(p, g, m0, v0, lazy=False, **kw)
    assert np.array_equal(md, A([[1.5, -1.5], [0.5, 0.5]])) and np.array_equal(vd, A([[2.25, 2.25], [3, 3]]))
    d = np.sqrt(f32(3)) / f32(0.5) + f32(1)
    want = f32(3) + f32(-1) * (f32(0.5) / d)
    assert pd[1, 0] == want and pd[1, 0] < 3 and np.array_equal(pd[0], p1[0])


def test_negative_zero_row_is_untouched_and_nan_row_is_touched():
    p = A([[1, 2], [3, 4]])
    g = A([[-0.0, 0.0], [np.nan, 0.0]])
    assert R.touched_rows(g).tolist() == [False, True]
    m0, v0 = A([[1, 1], [1, 1]]), A([[4, 4], [4, 4]])
    p1, m1, v1 = R.adam(p, g, m0, v0, t=3, lr=0.1, lazy=True)
    for new, old in ((p1, p), (m1, m0), (v1, v0)):
        assert np.array_equal(R.bits(new[0]), R.bits(old[0]))          # -0.0 everywhere: not touched
    assert np.isnan(p1[1, 0]) and np.isnan(m1[1, 0]) and np.isnan(v1[1, 0])        # the NaN row was updated
    assert p1[1, 1] != p[1, 1] and not np.isnan(p1[1, 1])                          # ... all of it: its finite column moved


def test_step_dispatch_creates_zero_state():
    p, g = A([[1, 2], [3, 4]]), A([[0.5, -1], [0, 0]])
    p1, st = R.step("adam", p, g, {}, 1, lr=0.1)
    want = R.adam(p, g, np.zeros_like(p), np.zeros_like(p), 1, 0.1)
    assert np.array_equal(p1, want[0]) and np.array_equal(st["exp_avg"], want[1]) and np.array_equal(st["exp_avg_sq"], want[2])
    assert set(R.STATE_KEYS) == set(R.KINDS) == set(_C.OPTIM_KINDS)
    for k in R.KINDS:
        assert len(R.STATE_KEYS[k]) == _C.OPTIM_STATES[k]


# ------------------------------------------------------------------------------------------- the restatement and torch
M_T, K_T, STEPS_T, FRACTION_T = 4096, 28, 25, 0.3
CASES = {"sgd": (torch.optim.SGD, dict(lr=0.1)), "sgd_momentum": (torch.optim.SGD, dict(lr=0.1, momentum=0.9)),
         "rmsprop": (torch.optim.RMSprop, dict(lr=1e-2)), "adam": (torch.optim.Adam, dict(lr=1e-2))}


def torch_inputs(M=M_T, K=K_T, steps=STEPS_T, fraction=FRACTION_T, seed=0):
    """(p0 float32 [M, K], grads: `steps` float32 [M, K] with `fraction` of the rows touched, per-row scales 1e-6 .. 1)."""
    rng = np.random.default_rng(seed)
    p0 = rng.standard_normal((M, K)).astype(np.float32)
    scale = (10.0 ** rng.uniform(-6.0, 0.0, size=(M, 1))).astype(np.float32)
    grads = []
    for _ in range(steps):
        live = rng.random((M, 1)) < fraction
        grads.append((rng.standard_normal((M, K)).astype(np.float32) * scale * live).astype(np.float32))
    return p0, grads


def run_torch(kind, dtype, lazy, p0, grads, device="cpu"):
    """torch.optim's optimizer of the same name; lazy: the untouched rows of the parameter and of every state table are
    put back after each step.  Returns (p, {state key: table}) as float64 numpy."""
    cls, kw = CASES[kind]
    p = torch.tensor(p0, dtype=dtype, device=device).requires_grad_(True)
    opt = cls([p], **kw)
    for g in grads:
        p.grad = torch.tensor(g, dtype=dtype, device=device)
        keep = torch.as_tensor(~R.touched_rows(g), device=device)
        before = {k: v.clone() for k, v in opt.state[p].items() if k != "step" and torch.is_tensor(v)}
        p_before = p.detach().clone()
        opt.step()
        if lazy:
            with torch.no_grad():
                p[keep] = p_before[keep]
                for k, v in opt.state[p].items():
                    if k != "step" and torch.is_tensor(v):
                        v[keep] = before[k][keep] if k in before else 0        # created by this step: it was zero
    state = {k: v.detach().double().cpu().numpy() for k, v in opt.state[p].items() if k != "step" and torch.is_tensor(v)}
    return p.detach().double().cpu().numpy(), state


def run_restatement(kind, lazy, p0, grads):
    _, kw = CASES[kind]
    p, state = p0.copy(), {}
    for t, g in enumerate(grads, 1):
        p, state = R.step(kind, p, g, state, t, lazy=lazy, **kw)
    return p, state


def deviations(got_p, got_state, truth_p, truth_state):
    out = {"p": float(np.abs(got_p.astype(np.float64) - truth_p).max())}
    for k, v in got_state.items():
        out[k] = float(np.abs(np.asarray(v, np.float64) - truth_state[k]).max())
    return out


@pytest.mark.parametrize("lazy", [False, True], ids=["dense", "lazy"])
@pytest.mark.parametrize("kind", list(CASES))
def test_restatement_against_torch_float64(kind, lazy):
    """Truth: torch's optimizer in float64.  The restatement's max |deviation| must be within 2x that of the same torch
    optimizer run in float32: both are float32 rounding sequences of the same length, which differ only in fused
    multiply-adds and in torch's lerp.  (The two float32 results are not bit-equal, hence the float64 yardstick.)"""
    p0, grads = torch_inputs()
    truth_p, truth_s = run_torch(kind, torch.float64, lazy, p0, grads)
    t32_p, t32_s = run_torch(kind, torch.float32, lazy, p0, grads)
    got_p, got_s = run_restatement(kind, lazy, p0, grads)
    ours, theirs = deviations(got_p, got_s, truth_p, truth_s), deviations(t32_p, t32_s, truth_p, truth_s)
    same = float((got_p == t32_p.astype(np.float32)).mean())
    for key in ours:
        print(f"{kind} {'lazy' if lazy else 'dense'} {key}: restatement {ours[key]:.3e}  torch float32 {theirs[key]:.3e}  "
              f"ratio {ours[key] / max(theirs[key], 1e-300):.3f}" + (f"  equal elements {100 * same:.1f} %" if key == "p" else ""))
    for key in ours:
        assert ours[key] <= 2.0 * theirs[key], (kind, lazy, key, ours[key], theirs[key])
    if lazy:        # and the untouched rows of the last step kept their bits
        prev_p, _ = run_restatement(kind, lazy, p0, grads[:-1])
        keep = ~R.touched_rows(grads[-1])
        assert keep.any() and np.array_equal(R.bits(got_p[keep]), R.bits(prev_p[keep]))


# ------------------------------------------------------------------------------------------------------ the C surface
def test_symbols_and_abi_version():
    lib = ctypes.CDLL(_C.LIB_PATH)
    for name in ("svoxt_optim_step", "svoxt_optim_state_count"):
        assert name in _C.EXPORTS and hasattr(lib, name)
    assert lib.svoxt_abi_version() == _C.ABI_VERSION == 22
    assert [_abi._lib.svoxt_optim_state_count(k) for k in (0, 1, 2, 3, 4, -1)] == [0, 1, 1, 2, -1, -1]
    assert ctypes.sizeof(_abi._COptimHyper) == 28


def test_c_entry_refuses_bad_arguments_before_any_launch():
    """Every call here returns SVOXT_ERR_INVALID from the argument checks: nothing reaches the HIP runtime (there is no GPU)."""
    step, h = _abi._lib.svoxt_optim_step, _abi._COptimHyper()
    P, G, S1, S2 = 0x1000, 0x2000, 0x3000, 0x4000            # never dereferenced: refused first
    bad = {
        "unknown kind": (7, P, G, S1, S2, 4, 4, h, 1, None),
        "negative kind": (-1, P, G, S1, S2, 4, 4, h, 1, None),
        "null param": (0, None, G, None, None, 4, 4, h, 1, None),
        "null grad": (0, P, None, None, None, 4, 4, h, 1, None),
        "momentum without its buffer": (1, P, G, None, None, 4, 4, h, 1, None),
        "rmsprop without its table": (2, P, G, None, None, 4, 4, h, 1, None),
        "adam without state2": (3, P, G, S1, None, 4, 4, h, 1, None),
        "M = 0": (0, P, G, None, None, 0, 4, h, 1, None),
        "K = 0": (0, P, G, None, None, 4, 0, h, 1, None),
        "M * K too large": (0, P, G, None, None, 1 << 36, 2, h, 1, None),
        "more than 2^32 lanes, K = 4 (one lane a row)": (0, P, G, None, None, 1 << 32, 4, h, 1, None),
        "more than 2^32 lanes, K = 32 (8 lanes a row)": (0, P, G, None, None, 1 << 29, 32, h, 1, None),
        "more than 2^32 lanes, K = 31 (32 lanes a row)": (0, P, G, None, None, 1 << 27, 31, h, 1, None),
        "lazy = 2": (0, P, G, None, None, 4, 4, h, 2, None),
        "param is grad": (0, P, P, None, None, 4, 4, h, 1, None),
        "state1 is state2": (3, P, G, S1, S1, 4, 4, h, 1, None),
        "misaligned": (0, P + 2, G, None, None, 4, 4, h, 1, None),
    }
    for what, args in bad.items():
        assert step(*args) == 1, what
        assert b"svoxt_optim_step" in _abi._lib.svoxt_last_error(), what


def test_operator_refuses_bad_arguments_before_any_launch():
    p, g = torch.zeros(4, 4), torch.zeros(4, 4)
    s1, s2 = torch.zeros(4, 4), torch.zeros(4, 4)
    h = {"neg_step": -0.1}
    cases = [
        ("kind must be", lambda: _C.optim_step("adagrad", p, g, None, None, h, True)),
        ("state1 must be given", lambda: _C.optim_step("adam", p, g, None, s2, h, True)),
        ("state2 must be given", lambda: _C.optim_step("adam", p, g, s1, None, h, True)),
        ("state1 must be None", lambda: _C.optim_step("sgd", p, g, s1, None, h, True)),
        ("state2 must be None", lambda: _C.optim_step("rmsprop", p, g, s1, s2, h, True)),
        ("param must be a dense float32", lambda: _C.optim_step("sgd", p.double(), g, None, None, h, True)),
        ("grad must be a dense float32", lambda: _C.optim_step("sgd", p, g.half(), None, None, h, True)),
        ("grad must be a dense float32", lambda: _C.optim_step("sgd", p, g.to_sparse(), None, None, h, True)),
        ("grad must be a dense float32", lambda: _C.optim_step("sgd", p, None, None, None, h, True)),
        ("param must be [M, K]", lambda: _C.optim_step("sgd", p.reshape(-1), g.reshape(-1), None, None, h, True)),
        ("param must be [M, K]", lambda: _C.optim_step("sgd", p[:0], g[:0], None, None, h, True)),
        ("grad must have the shape", lambda: _C.optim_step("sgd", p, g[:2], None, None, h, True)),
        ("state1 must have the shape", lambda: _C.optim_step("rmsprop", p, g, s1[:, :2], None, h, True)),
        ("grad must be contiguous", lambda: _C.optim_step("sgd", p, g.t(), None, None, h, True)),
        ("param must be contiguous", lambda: _C.optim_step("sgd", torch.zeros(4, 8)[:, ::2], g, None, None, h, True)),
        ("hyper must be a dict", lambda: _C.optim_step("sgd", p, g, None, None, {"lr": 0.1}, True)),
        ("hyper must be a dict", lambda: _C.optim_step("sgd", p, g, None, None, 0.1, True)),
        ("must be a CUDA tensor", lambda: _C.optim_step("sgd", p, g, None, None, h, True)),       # all else in order: no CPU path
    ]
    for text, call in cases:
        with pytest.raises(RuntimeError, match=text.replace("[", r"\[").replace("]", r"\]")):
            call()
    assert p._version == 0 and s1._version == 0              # nothing was written, nothing was claimed written


# -------------------------------------------------------------------------------------------------- the Python surface
CLASSES = {"FeatureSGD": FO.FeatureSGD, "FeatureRMSprop": FO.FeatureRMSprop, "FeatureAdam": FO.FeatureAdam}


def test_classes_are_exported_and_gpu_only():
    for name, cls in CLASSES.items():
        assert name in svox_t_amd.__all__ and getattr(svox_t_amd, name) is cls
        assert issubclass(cls, torch.optim.Optimizer)
        with pytest.raises(RuntimeError, match="parameter 0 of group 0 must be on a GPU"):
            cls([torch.zeros(4, 4, requires_grad=True)], lr=0.1)


def test_unsupported_options_are_refused():
    p = [torch.zeros(4, 4, requires_grad=True)]
    refused = [
        (FO.FeatureSGD, dict(lr=0.1, weight_decay=1e-4), "weight_decay"), (FO.FeatureSGD, dict(lr=0.1, momentum=0.9, nesterov=True), "nesterov"),
        (FO.FeatureSGD, dict(lr=0.1, momentum=0.9, dampening=0.1), "dampening"), (FO.FeatureSGD, dict(lr=0.1, maximize=True), "maximize"),
        (FO.FeatureRMSprop, dict(weight_decay=1e-4), "weight_decay"), (FO.FeatureRMSprop, dict(centered=True), "centered"),
        (FO.FeatureRMSprop, dict(momentum=0.9), "momentum"), (FO.FeatureRMSprop, dict(maximize=True), "maximize"),
        (FO.FeatureAdam, dict(weight_decay=1e-4), "weight_decay"), (FO.FeatureAdam, dict(amsgrad=True), "amsgrad"),
        (FO.FeatureAdam, dict(maximize=True), "maximize"),
    ]
    for cls, kw, word in refused:
        with pytest.raises(RuntimeError, match=f"does not implement {word}"):
            cls(p, **kw)
    for cls, kw in ((FO.FeatureSGD, dict(lr=-1.0)), (FO.FeatureAdam, dict(betas=(0.9, 1.0))), (FO.FeatureAdam, dict(eps=-1.0)),
                    (FO.FeatureRMSprop, dict(alpha=-0.1)), (FO.FeatureAdam, dict(lr=torch.tensor(0.1)))):
        with pytest.raises(RuntimeError, match="invalid|Python number"):
            cls(p, **kw)


def test_parameter_checks_name_the_parameter():
    good = torch.zeros(4, 4, requires_grad=True)
    for bad in (torch.zeros(4, 4, dtype=torch.float64, requires_grad=True), torch.zeros(16, requires_grad=True)):
        with pytest.raises(RuntimeError, match="parameter 0 of group 1 must be a dense float32"):
            FO.FeatureAdam([{"params": []}, {"params": [bad, good]}])


@pytest.fixture
def faked(monkeypatch):
    """The optimizers on CPU tensors: the GPU-only check off, the two operators replaced by recorders / torch indexing."""
    calls = []
    monkeypatch.setattr(FO, "_check_table", lambda p, what: None)
    monkeypatch.setattr(_C, "optim_step", lambda kind, p, g, s1, s2, hyper, lazy: calls.append((kind, p, g, s1, s2, dict(hyper), lazy)))
    monkeypatch.setattr(_C, "gather_rows", lambda table, row_map: table[row_map].clone())
    return calls


def test_step_bookkeeping_with_a_faked_kernel(faked):
    p = torch.zeros(4, 4, requires_grad=True)
    q = torch.zeros(2, 4, requires_grad=True)
    opt = FO.FeatureAdam([p, q], lr=0.25, betas=(0.5, 0.75), eps=1.0, lazy=False)
    p.grad = torch.ones(4, 4)
    assert opt.step(lambda: 7.0) == 7.0                      # the closure's value comes back; q has no grad: skipped
    opt.step()
    assert len(faked) == 2 and q not in opt.state
    (k1, p1, g1, m1, v1, h1, lazy1), (_, _, _, m2, v2, h2, _) = faked
    assert k1 == "adam" and p1 is p and g1 is p.grad and lazy1 is False
    st = opt.state[p]
    assert set(st) == {"step", "exp_avg", "exp_avg_sq"} and m1 is st["exp_avg"] and v2 is st["exp_avg_sq"] and m2 is m1
    assert float(st["step"]) == 2.0 and st["step"].dtype == torch.float32 and not st["step"].is_cuda
    assert not m1.any() and m1.shape == p.shape
    # the scalars: double precision, t = 1 then 2
    assert h1 == {"neg_step": -0.25 / (1 - 0.5), "one_minus_beta1": 0.5, "beta2": 0.75, "one_minus_beta2": 0.25,
                  "bias2_sqrt": math.sqrt(1 - 0.75), "eps": 1.0}
    assert h2["neg_step"] == -0.25 / (1 - 0.25) and h2["bias2_sqrt"] == math.sqrt(1 - 0.75 ** 2)
    # an lr scheduler's write is read by the next step
    opt.param_groups[0]["lr"] = 0.5
    opt.step()
    assert faked[-1][5]["neg_step"] == -0.5 / (1 - 0.5 ** 3)
    # kinds and state keys of the others
    for cls, kw, kind, keys in ((FO.FeatureSGD, dict(lr=0.1), "sgd", set()), (FO.FeatureSGD, dict(lr=0.1, momentum=0.9), "sgd_momentum", {"momentum_buffer"}),
                                (FO.FeatureRMSprop, dict(lr=0.1), "rmsprop", {"square_avg"})):
        o = cls([p], **kw)
        o.step()
        assert faked[-1][0] == kind and faked[-1][6] is True and set(o.state[p]) - {"step"} == keys
    assert faked[-1][5] == {"neg_step": -0.1, "beta2": 0.99, "one_minus_beta2": 1.0 - 0.99, "eps": 1e-8}
    # a sparse gradient is refused
    p.grad = torch.ones(4, 4).to_sparse()
    with pytest.raises(RuntimeError, match="parameter 0 of group 0: a sparse gradient"):
        opt.step()


def test_state_dict_moves_to_and_from_torch(faked):
    p = torch.zeros(4, 4, requires_grad=True)
    opt = FO.FeatureAdam([p], lr=0.1)
    p.grad = torch.ones(4, 4)
    opt.step()
    opt.state[p]["exp_avg"].fill_(3.0)
    theirs = torch.optim.Adam([p], lr=0.1)
    theirs.load_state_dict(opt.state_dict())
    assert float(theirs.state[p]["step"]) == 1.0 and float(theirs.state[p]["exp_avg"][0, 0]) == 3.0
    theirs.step()                                            # torch accepts the state as its own
    back = FO.FeatureAdam([p], lr=0.1)
    back.load_state_dict(theirs.state_dict())
    back.step()
    assert float(back.state[p]["step"]) == 3.0 and faked[-1][3] is back.state[p]["exp_avg"]
    # a torch state dict with an option these do not implement is refused at the next step, not ignored
    back.load_state_dict(torch.optim.Adam([p], lr=0.1, amsgrad=True).state_dict())
    with pytest.raises(RuntimeError, match="amsgrad"):
        back.step()


@pytest.mark.parametrize("name", ["adam", "sgd_momentum", "rmsprop", "sgd"])
def test_a_state_dict_born_in_torch_loads_and_steps(faked, name):
    """The checkpoint of a run that used torch.optim: its param groups have no `lazy`; the constructor's value holds."""
    torch_cls, kw = CASES[name]
    ours_cls = {"adam": FO.FeatureAdam, "rmsprop": FO.FeatureRMSprop}.get(name, FO.FeatureSGD)
    p = torch.zeros(4, 4, requires_grad=True)
    theirs = torch_cls([p], **kw)
    p.grad = torch.ones(4, 4)
    theirs.step()
    saved = theirs.state_dict()
    assert "lazy" not in saved["param_groups"][0]
    for lazy in (True, False):
        ours = ours_cls([p], lazy=lazy, **{**kw, "lr": 0.5})
        ours.load_state_dict(saved)
        assert ours.param_groups[0]["lazy"] is lazy and ours.param_groups[0]["lr"] == kw["lr"]      # saved options win, lazy is ours
        ours.step()
        kind, _, _, s1, s2, hyper, was_lazy = faked[-1]
        assert kind == name and was_lazy is lazy and hyper["neg_step"] == (-kw["lr"] if name != "adam" else -kw["lr"] / (1 - 0.9 ** 2))
        keys = R.STATE_KEYS[name]
        for tab, k in zip((s1, s2), keys):
            assert tab is ours.state[p][k] and torch.equal(tab, theirs.state[p][k])
        if "step" in theirs.state[p]:
            assert float(ours.state[p]["step"]) == 2.0
    import copy
    revived = copy.deepcopy(ours)                             # __setstate__ alone (pickling) keeps the groups whole too
    assert revived.param_groups[0]["lazy"] is False


def test_rebind_bookkeeping(faked):
    old = torch.nn.Parameter(torch.zeros(5, 4))
    other = torch.nn.Parameter(torch.zeros(3, 4))
    opt = FO.FeatureAdam([{"params": [other]}, {"params": [old], "lr": 0.5}], lr=0.1)
    old.grad = torch.ones(5, 4)
    opt.step()
    m = opt.state[old]["exp_avg"]
    m.copy_(torch.arange(20.).reshape(5, 4))
    row_map = torch.tensor([4, 0, 2])
    new = torch.nn.Parameter(torch.zeros(3, 4))
    opt.rebind(old, new, row_map)
    assert opt.param_groups[1]["params"] == [new] or opt.param_groups[1]["params"][0] is new
    assert opt.param_groups[1]["lr"] == 0.5 and opt.param_groups[0]["params"][0] is other
    assert old not in opt.state and float(opt.state[new]["step"]) == 1.0
    assert torch.equal(opt.state[new]["exp_avg"], m[row_map]) and opt.state[new]["exp_avg_sq"].shape == (3, 4)
    # without a row_map: fresh state
    newer = torch.nn.Parameter(torch.zeros(7, 4))
    opt.rebind(new, newer)
    assert opt.param_groups[1]["params"][0] is newer and new not in opt.state and newer not in opt.state
    newer.grad = torch.ones(7, 4)
    opt.step()
    assert float(opt.state[newer]["step"]) == 1.0 and not opt.state[newer]["exp_avg"].any()
    # refusals leave everything as it was
    stranger = torch.nn.Parameter(torch.zeros(7, 4))
    for args, text in (((stranger, new), "not a parameter of this optimizer"), ((newer, other), "already a parameter"),
                       ((newer, new, torch.tensor([0, 1])), "row_map"), ((newer, new, torch.tensor([0, 1, 7])), "outside the old table"),
                       ((newer, new, torch.tensor([0, 1, 2], dtype=torch.int32)), "int64"),
                       ((newer, torch.nn.Parameter(torch.zeros(3, 5)), torch.tensor([0, 1, 2])), "row_map")):
        with pytest.raises(RuntimeError, match=text):
            opt.rebind(*args)
        assert opt.param_groups[1]["params"][0] is newer and newer in opt.state
