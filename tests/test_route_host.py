"""The routes of the colour render step without a GPU: svox_t_amd.csrc._fwd_route and _bwd_route -- pure functions of the
packed structs and the switches ("One route record for the render step") -- held to what the host did BEFORE
its decisions were records: tests/golden/route_labels.json, recorded on the GPU from that commit by
tests/golden/make_route_golden.py over every (payload, batch, route, fast) of tests/test_gpu_route_matrix.py at seed 0.

The structs are filled by hand as tests/test_placement_host.py fills its own (the addresses are never dereferenced: the two
queries of the library the routes ask, svoxt_can_record and svoxt_fwd_fills_terms, read fields); what the layers above the
executors do to a call -- the padded and grouped payloads, the plan a forward leaves, sort_rays -- is restated in `calls`
below from the payload's configuration and the switches alone.  For every entry the forward's route, the list facts it
states and the backward's route that follows from them must give

    the golden's labels, character for character, and its forward_terms;
    the golden's ordered names of library entry points (ray order, mask / table build, the entry itself, the compaction);
    the prefixes tests/test_gpu_route_matrix.py::KERNELS means each switch to select (at thresholds 0, as there).

No entry may be skipped: the entries reproduced are counted against the file's own count."""
import ctypes
import os
import sys
import types

import pytest

import svox_t_amd as svox
import svox_t_amd.csrc as _C
from svox_t_amd.csrc import _abi
from tests import test_gpu_route_matrix as G
from tests.test_route_matrix_host import FAR, INSIDE, PAYLOADS, Q

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden"))
import make_route_golden as GOLDEN  # noqa: E402

BASE = 0x10000                      # never dereferenced
IMAGES = {"ragged": None, "inside": (INSIDE["height"], INSIDE["width"]), "far": (FAR["height"], FAR["width"])}
M = 15000
# every switch a route reads, at the value the golden was recorded with (the environment may say otherwise here)
DEFAULTS = dict(BWD_EXACT=True, NATIVE_MATH=False, SIGMA_MASK=True, BWD_LIST_SAMPLES=96, FWD_LIST_SAMPLES=96, LIST_POOL=True,
                AUTO_PLAN=True, FWD_SPLIT="", BWD_GATHER=1, FWD_OVERLAP=True, EXP_TABLE=True, BWD_TERMS=True, BWD_FUSED=True,
                BWD_XF_FUSED=True, ROLES_FLAGS=0, GRAD_SCRATCH=True, PAD_PAYLOADS=True, GROUP_PAYLOADS=True)


def _tree(K, N, xf, accel):
    t = _abi._CTree()
    t.features, t.M, t.K, t.N = BASE, M, K, N
    t.data, t.child, t.n_internal, t.offset, t.scaling = 2 * BASE, 3 * BASE, 3000, 4 * BASE, 5 * BASE
    if xf:
        t.xform, t.xform_dim = 6 * BASE, 4
    if accel:
        t.accel, t.accel_log2 = 7 * BASE, 5
    return t


def _rays(image):
    r = _abi._CRays()
    r.origins = r.dirs = r.vdirs = 8 * BASE
    r.Q = Q if image is None else image[0] * image[1]
    if image is not None:
        r.image_height, r.image_width = image
    return r


def _opts(fmt, bd, fast):
    th = 1e-2 if fast else 0.0
    return _abi._COptions(1e-3, 1.0, fmt, bd, -1, -1, 0.0, 0, max(bd - 1, 0), th, th)


def calls(payload, sw):
    """[(K, columns of grad_output)] of the executor calls one volume_render makes for a payload: itself, as the next
    specialised payload (PAD_PAYLOADS), or in groups of three channels, the short last group padded (GROUP_PAYLOADS)."""
    cfg = PAYLOADS[payload]
    df = svox.DataFormat(cfg["fmt"])
    K, bd = cfg["K"], max(df.basis_dim, 1)
    rgba = df.format == _abi.FORMAT_RGBA
    cols = K if rgba else (K - 1) // bd + 1
    if payload in ("rgba6", "sh4_two") and sw.get("PAD_PAYLOADS", True):
        return [(8, 8)] if rgba else [(3 * bd + 1, 4)]
    if payload == "sh4_four" and sw.get("GROUP_PAYLOADS", True):
        return [(3 * bd + 1, 4)] * 2          # (channels 0 .. 2; channel 3, padded -- unless PAD_PAYLOADS is off, which no route here asks)
    return [(K, cols)]


def reproduce(mp, payload, batch, name, fast, sw, kw, want):
    """The problems of one golden entry (none: reproduced)."""
    cfg, image = PAYLOADS[payload], IMAGES[batch]
    df = svox.DataFormat(cfg["fmt"])
    persp = name == GOLDEN.PERSP
    said = types.SimpleNamespace(coherent=bool(kw.get("sort_rays")))           # (_in_coherent_order: 2048 rays are sorted on request alone)
    accel = cfg["N"] == 2 and sw.get("ACCEL_LOG2") != 0
    got = {k: None for k in want}
    fwd_calls, bwd_calls, second_calls, ng_calls = [], [], [], []
    with mp.context() as m:
        for k, v in {**DEFAULTS, **sw}.items():
            if k not in ("_dry", "_again", "ACCEL_LOG2", "ACCEL_BRICKS"):
                m.setattr(_C, k, v)
        for K, cols in calls(payload, sw):
            ct, cr, co = _tree(K, cfg["N"], bool(cfg.get("xf")), accel), _rays(image), _opts(df.format, df.basis_dim, fast)
            coherent = _C._coherent(cr, said)
            assert coherent == (image is not None or said.coherent)
            order = ["svoxt_ray_order"] if said.coherent else []
            stride_is_K = K <= 8 or K % 16 == 0

            def forward(record):
                r = _C._fwd_route(ct, cr, co, record, coherent, accel, bool(_C.SIGMA_MASK))
                assert isinstance(r, _C._FwdRoute) and r.entry in (_C._FWD_RECORD, _C._FWD_SCRATCH, _C._FWD_WS, _C._FWD)
                build = [] if not r.mask else ["svoxt_exp_table_build"] if r.mask_table else \
                    ["svoxt_sigma_mask_build_fill" if (r.record and _C.LIST_POOL) else "svoxt_sigma_mask_build"]
                return r, order + build + [r.entry]

            def backward(lists, has_fo):
                r = _C._bwd_route(ct, co, cols, coherent, lists, has_fo)
                assert isinstance(r, _C._BwdRoute) and r.replay == (r.kind != "march")
                compact = [] if stride_is_K else ["svoxt_compact_rows_clear" if (_C.GRAD_SCRATCH and r.replay) else "svoxt_compact_rows"]
                return r, ["svoxt_volume_render_bwd_replay" if r.replay else "svoxt_volume_render_bwd"] + compact

            if want["forward"] is not None:
                # a plain call whose features require a gradient records for the plan it leaves (AUTO_PLAN), else renders only
                f, c = forward(record=bool(_C.AUTO_PLAN))
                fwd_calls += c
                lists = f.list_facts()
                assert (lists is not None) == f.record and (lists is None or lists.terms_state == f.fills)
                b, c = backward(lists, has_fo=lists is not None)                # (the plan hands the forward's output with its lists)
                bwd_calls += c
                got.update(forward=f.label, forward_terms=f.forward_terms, backward=b.label)
                if want["second_backward"] is not None:                           # the plan served one backward: this one has no lists
                    b2, c = backward(None, False)
                    second_calls += c
                    got["second_backward"] = b2.label
            if want["no_grad_forward"] is not None:
                f, c = forward(record=False)
                ng_calls += c
                got["no_grad_forward"] = f.label
    got.update(forward_calls=fwd_calls or None, backward_calls=bwd_calls or None, second_backward_calls=second_calls or None,
               no_grad_calls=ng_calls or None)
    problems = [f"{k}: got {got[k]!r}, golden {want[k]!r}" for k in want if got[k] != want[k]]
    if not fast and sw.get("PAD_PAYLOADS") is not False and sw.get("GROUP_PAYLOADS") is not False:
        fam, coh = G.FAMILY[payload], image is not None or said.coherent or persp
        for side, label, prefix in (("forward", got["forward"], G.KERNELS(fam, coh, sw)[0]),
                                    ("backward", got["backward"], G.KERNELS(fam, coh, sw)[1]),
                                    ("second backward", got["second_backward"], G.MARCH),
                                    ("no_grad forward", got["no_grad_forward"], G.KERNELS(fam, coh, sw, grad=False)[0])):
            if label is not None and prefix is not None and not label.startswith(prefix):
                problems.append(f"{side} took {label!r}, meant {prefix!r}")
    return problems


def switches_of(payload, batch):
    """route name -> (switches, keywords of forward), as tests/test_gpu_route_matrix.py::routes gives them."""
    a = types.SimpleNamespace(payload=payload, image=IMAGES[batch])
    out = {name: (sw, kw) for name, sw, kw in G.routes(a)}
    out[GOLDEN.SCRATCH4] = ({"FWD_LIST_SAMPLES": 4}, {})
    out[GOLDEN.PERSP] = ({}, {})
    return out


def test_the_queries_of_the_routes_read_fields_only():
    """Hand-filled structs with dummy addresses go through both host-only queries (nothing is dereferenced)."""
    t, o = _tree(13, 2, True, False), _opts(_abi.FORMAT_SH, 4, False)
    assert _abi._lib.svoxt_can_record(ctypes.byref(t), ctypes.byref(o)) == 1
    assert _abi._lib.svoxt_fwd_fills_terms(ctypes.byref(t), ctypes.byref(o), _abi.LISTS_FWD_TWO_KERNELS) == 3
    assert _abi._lib.svoxt_fwd_fills_terms(ctypes.byref(t), ctypes.byref(o), 0) == 0
    t, o = _tree(28, 2, False, True), _opts(_abi.FORMAT_SG, 9, False)
    assert _abi._lib.svoxt_can_record(ctypes.byref(t), ctypes.byref(o)) == 2


def test_every_golden_entry_is_reproduced(monkeypatch):
    doc, entries = GOLDEN.read()
    assert doc["seed"] == 0 and len(entries) == doc["count"] > 2000
    assert {p for p, *_ in entries} == set(PAYLOADS) and {b for _, b, *_ in entries} == set(IMAGES)
    table, problems, done = {}, [], 0
    for payload, batch, name, fast, want in entries:
        if (payload, batch) not in table:
            table[payload, batch] = switches_of(payload, batch)
        sw, kw = table[payload, batch][name]           # (a name the matrix does not yield is a KeyError, not a skip)
        for p in reproduce(monkeypatch, payload, batch, name, fast, sw, kw, want):
            problems.append(f"{payload}/{batch} {name}{' fast' if fast else ''}: {p}")
        done += 1
    # every route of the matrix is in the file, and nothing else but the two walks that are no route
    for (payload, batch), routes in table.items():
        seen = {n for p, b, n, *_ in entries if (p, b) == (payload, batch)}
        assert seen <= set(routes) and set(routes) - seen <= {GOLDEN.PERSP}, (payload, batch, set(routes) ^ seen)
    assert done == doc["count"], f"{done} of {doc['count']} entries reproduced"
    assert not problems, f"{len(problems)} problems:\n" + "\n".join(problems[:40])


@pytest.mark.parametrize("name", ["LAST_ROUTE", "_volume_render", "_take_plan", "_planned_forward", "_pool_blocks_for", "_POOL_HINT",
                                  "_detect_image", "_IMAGE_TRUST", "_IMAGE_SHAPES", "_SIGMA_CACHE", "_GRAD_SCRATCH", "_ray_order32",
                                  "_in_coherent_order", "SampleLists", "features_held", "invalidate_caches", "freeze_pools"]
                         + list(DEFAULTS))
def test_what_tests_and_the_benchmark_reach_into_is_still_there(name):
    assert hasattr(_C, name)
    if name in DEFAULTS and name not in ("BWD_EXACT", "NATIVE_MATH"):           # (the two the environment may set)
        assert getattr(_C, name) == DEFAULTS[name]
    if name == "LAST_ROUTE":
        assert set(_C.LAST_ROUTE) == {"forward", "backward", "forward_terms"}
