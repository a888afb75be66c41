"""The shade's record staging (shade_tile_body, svoxt_fwd_kernels.h): a tile's list blocks go into a ring of nine
blocks in LDS before the first round -- 72 list positions; six blocks in the kernels that shade from memory a finished
launch left -- and a block a round has used up is replaced by its successor a ring's length on, so that a gathering
wavefront reads its record from LDS and requests the row at once.

What can go wrong is in the indexing: the window's slots, the column swizzle, rounds of 7 positions that straddle
blocks of 8, the refill of lists longer than the window, lists that end on a block boundary, a partial last tile,
lists cut short by their capacity.  Each scene goes through the one-launch forward (fwd_roles_kernel) and the
two-launch form (march_rec_kernel + shade_tile_kernel): pixels bit for bit against the CPU oracle, list headers,
records and hand-over equal between the two in the canonical form, the gradient within the hand-over test's tolerance;
then with thresholds, without recording, and with the "stale record" test flag, whose tiles the fallback launch
(fwd_finish_kernel -- the third caller) shades again.  Every test asserts from the list lengths that its scene has
the tiles it claims: a scene that stops exercising the refill fails.

One test without a GPU compiles the headline instance and holds it to three workgroups per CU."""
import functools
import os
import re
import shutil
import subprocess

import numpy as np
import pytest
import torch

import svox_t_amd as svox
import svox_t_amd.csrc as _C
from oracle import oracle as O
from svox_t_amd import synth
from svox_t_amd.renderer import _rays_spec_from_rays
from tests.test_gpu_roles_handoff import _canonical, _counters
from tests.util import Case

WINDOW = 72          # list positions the staging window of fwd_roles_kernel holds (kShadeWin * 8); shade_tile_kernel and
                     # fwd_finish_kernel take kShadeWinSmall * 8 = 48: a list beyond 72 refills the ring at either size

# name -> (case, image?, a lower bound on the tiles whose longest list exceeds the window, what else the scene must show)
SCENES = {
    "d8_sh9_image": (dict(depth=8, K=28, data_format="SH9", width=64, height=64), True, 1),
    "d7_sh9_image": (dict(depth=7, K=28, data_format="SH9", width=64, height=64), True, 0),       # (beyond the small window only)
    "d6_sh4_ragged": (dict(depth=6, K=13, data_format="SH4", width=203, height=77), False, 0),
    "d5_rgba4_image": (dict(depth=5, K=4, data_format="RGBA", width=64, height=48), True, 0),
}


@functools.lru_cache(maxsize=None)
def _case(name):
    return Case(**SCENES[name][0])


@functools.lru_cache(maxsize=None)
def _oracle_pixels(name, fast):
    c = _case(name)
    return O.volume_render(c.oracle_tree(), *c.rays_np(), c.oracle_opts(fast=fast))


def _setup(name, gpu, fast=False):
    kw, image, _ = SCENES[name]
    c = _case(name)
    # (the pooled lists size themselves by the forwards before them, per number of tiles and capacity: a pool sized
    # by another test's smaller scene would cut this scene's lists short -- right pixels, but not the lists under test)
    _C._POOL_HINT.clear()
    tree = c.tree(gpu)
    opt = svox.VolumeRenderer(tree)._get_options(fast=fast)
    spec = tree._spec(tree.features)
    shape = (kw["height"], kw["width"]) if image else None
    rs = _rays_spec_from_rays(c.rays_gpu(gpu), shape)
    rs.need_grad = False
    return c, tree, opt, spec, shape, rs


def _tile_longest(lists, shape, Q):
    """[tiles] the longest list of each tile, from the list headers (aux.x without its overflow flag)"""
    from tests.test_gpu_roles_handoff import _ray_of
    q = _ray_of(lists.tiles, shape, Q, lists.aux.device)
    n = torch.where(q >= 0, lists.aux[q.clamp(min=0), 0] & 0x7fffffff, torch.zeros_like(q))
    return n.max(dim=1).values, n


def _check_scene(name, lists, shape, Q, cap=None):
    """The scene has what the tests of this file rely on (the numbers are the CPU oracle's: oracle.ray_steps)."""
    longest, n = _tile_longest(lists, shape, Q)
    over = int((longest > WINDOW).sum())
    report = f"{name}: {lists.tiles} tiles, {int((longest > 0).sum())} busy, longest list {int(longest.max())}, {over} tiles beyond the window"
    if cap is not None:
        assert int(longest.max()) == cap and bool((lists.aux[:, 0].view(torch.int32) < 0).any()), f"{report}: no list reached its capacity"
        return report
    assert over >= SCENES[name][2], f"{report}: the scene no longer refills the ring"
    if name == "d8_sh9_image":
        assert int((longest > 40).sum()) > over, report                       # (lists between five blocks and the window too)
        assert int(longest.max()) >= WINDOW + 8, report                       # (the refill goes past its first block)
    if name == "d7_sh9_image":
        assert 48 < int(longest.max()) <= WINDOW, report                      # (inside the large window, a refill of the small one)
    if name == "d6_sh4_ragged":
        assert lists.tiles == 245 and Q % 64 != 0, report                     # (a partial last tile)
        assert bool(((n > 0) & (n % 8 == 0)).any()), f"{report}: no list ends on a block boundary"
        assert int(longest.max()) > 3 * 8, report
    return report


def _forward(spec, rs, opt):
    out, lists = _C.volume_render(spec, rs, opt, record=True)
    assert lists is not None and lists.terms is not None
    return out, lists


def _both_routes(name, gpu, monkeypatch, fast, cap=None):
    """A recording forward as two launches and as one: pixels against the oracle, everything else between the two."""
    c, tree, opt, spec, shape, rs = _setup(name, gpu, fast)
    g = synth.grad_output(c.Q, 4).to(gpu)
    monkeypatch.setattr(_C, "FWD_SPLIT", "1")
    monkeypatch.setattr(_C, "ROLES_FLAGS", 0)
    monkeypatch.setattr(_C, "FWD_OVERLAP", False)
    out0, l0 = _forward(spec, rs, opt)
    assert "fwd_roles_kernel" not in _C.LAST_ROUTE["forward"] and "shade_tile_kernel" in _C.LAST_ROUTE["forward"], _C.LAST_ROUTE
    report = _check_scene(name, l0, shape, c.Q, cap)
    np.testing.assert_array_equal(out0.cpu().numpy(), _oracle_pixels(name, fast), err_msg=f"{report}: two launches")
    want = _canonical(l0, shape, c.Q)
    grad0 = _C.volume_render_backward(spec, rs, opt, g, lists=l0)
    monkeypatch.setattr(_C, "FWD_OVERLAP", True)
    out1, l1 = _forward(spec, rs, opt)
    assert "fwd_roles_kernel" in _C.LAST_ROUTE["forward"], _C.LAST_ROUTE
    np.testing.assert_array_equal(out1.cpu().numpy(), _oracle_pixels(name, fast), err_msg=f"{report}: one launch")
    got = _canonical(l1, shape, c.Q)
    assert torch.equal(got[0], want[0]), f"{report}: aux"
    assert torch.equal(got[1], want[1]), f"{report}: records"
    assert want[2] is not None and torch.equal(got[2], want[2]), f"{report}: hand-over"
    shaded, mismatch, gaveup, dropped, fallback = _counters(l1)
    assert mismatch == 0 and shaded + fallback == want[3], (report, _counters(l1), want[3])
    grad1 = _C.volume_render_backward(spec, rs, opt, g, lists=l1)
    assert (grad1 - grad0).abs().max().item() <= 1e-6 * grad0.abs().max().item(), f"{report}: gradient"
    return report


@pytest.mark.gpu
@pytest.mark.parametrize("fast", [False, True], ids=["exact", "fast"])
@pytest.mark.parametrize("name", list(SCENES))
def test_recording_forward_both_routes(name, fast, gpu, monkeypatch, capsys):
    report = _both_routes(name, gpu, monkeypatch, fast)
    with capsys.disabled():
        print(f"\n[shade staging] {report}")


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SCENES))
def test_forward_without_recording(name, gpu, monkeypatch):
    """The scratch lists of a forward nobody differentiates: with thresholds the march applies the stop rule itself
    (march_rec_kernel<STOP> + shade_tile_kernel<STOP>), without them the one-launch forward runs."""
    c, tree, opt, spec, shape, rs = _setup(name, gpu)
    monkeypatch.setattr(_C, "FWD_SPLIT", "1")
    monkeypatch.setattr(_C, "ROLES_FLAGS", 0)
    # (the scene's claim, from a recording forward's list headers)
    _check_scene(name, _forward(spec, rs, opt)[1], shape, c.Q)
    for fast in (False, True):
        o = svox.VolumeRenderer(tree)._get_options(fast=fast)
        for overlap in (True, False):
            monkeypatch.setattr(_C, "FWD_OVERLAP", overlap)
            out = _C.volume_render(spec, rs, o)
            assert "shade_tile" in _C.LAST_ROUTE["forward"], _C.LAST_ROUTE
            np.testing.assert_array_equal(out.cpu().numpy(), _oracle_pixels(name, fast),
                                          err_msg=f"{name}: fast={fast}, one launch={overlap}: {_C.LAST_ROUTE['forward']}")


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SCENES))
def test_stale_records_are_caught_and_repaired(name, gpu, monkeypatch):
    """LISTS_TEST_STALE: the shading workgroup of every fifth tile treats the first record of each ray -- as read from
    the staging window -- as stale; its checksum must not match, and the fallback launch shades the tile again."""
    c, tree, opt, spec, shape, rs = _setup(name, gpu)
    monkeypatch.setattr(_C, "FWD_SPLIT", "1")
    monkeypatch.setattr(_C, "FWD_OVERLAP", True)
    monkeypatch.setattr(_C, "ROLES_FLAGS", 0)
    out0, l0 = _forward(spec, rs, opt)
    _check_scene(name, l0, shape, c.Q)
    want = _canonical(l0, shape, c.Q)
    monkeypatch.setattr(_C, "ROLES_FLAGS", _C.LISTS_TEST_STALE)
    out1, l1 = _forward(spec, rs, opt)
    assert "fwd_roles_kernel" in _C.LAST_ROUTE["forward"] and l1.flags & 0xf00 == _C.LISTS_TEST_STALE
    shaded, mismatch, gaveup, dropped, fallback = ctr = _counters(l1)
    assert mismatch > 0 and fallback >= mismatch and shaded + fallback == want[3], (ctr, want[3])
    np.testing.assert_array_equal(out1.cpu().numpy(), _oracle_pixels(name, False))
    assert torch.equal(out1, out0)
    got = _canonical(l1, shape, c.Q)
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1]) and torch.equal(got[2], want[2])


@pytest.mark.gpu
def test_capacity_below_the_longest_list(gpu, monkeypatch, capsys):
    """Lists of at most 48 positions where the longest would be over 80: every list that reaches the capacity is
    shaded to its end from the window and its ray marched on by the tail launch."""
    monkeypatch.setattr(_C, "BWD_LIST_SAMPLES", 48)
    report = _both_routes("d8_sh9_image", gpu, monkeypatch, False, cap=48)
    with capsys.disabled():
        print(f"\n[shade staging, capacity 48] {report}")


_HEADLINE = "fwd_roles_kernel<FMT_SH, 9, 1, true, false, false>"


@pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")
def test_headline_instance_keeps_three_workgroups_per_cu(tmp_path):
    """The one-launch forward of the headline workload (SH9, recording): no scratch, six wavefronts per SIMD -- three
    workgroups of eight per CU -- and an LDS footprint three of which fit a CU's 160 KiB."""
    from svox_t_amd import build as B
    src = tmp_path / "one_instance.hip"
    src.write_text(
        '#include <hip/hip_runtime.h>\n#include <stdint.h>\n#include <stdio.h>\n#include <stdlib.h>\n#include <string.h>\n'
        '#include "include/svoxt.h"\n#include "svoxt_device.h"\n#include "svoxt_host.h"\n#include "svoxt_launch.h"\n'
        '#include "svoxt_fwd_kernels.h"\n'
        f'namespace svoxt {{\ntemplate __global__ void {_HEADLINE}(TreeDev, RaysDev, Opts, RecLists, uint4*, float*, '
        'const uint32_t*, int32_t*, int, int, int, RolesMap);\n}\n')
    asm = tmp_path / "one_instance.s"
    root = os.path.dirname(os.path.dirname(B.CSRC))
    # (svoxt_kernels.hip includes the public header as "../../include/svoxt.h"; its guard makes the second inclusion empty)
    cmd = [B._hipcc()] + [f for f in B.HIPCC_FLAGS if f not in ("-shared", "-fPIC")] + \
        ["-I", B.CSRC, "-I", root, "-S", "--cuda-device-only", "-o", str(asm), str(src)]
    res = subprocess.run(cmd, stderr=subprocess.PIPE, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    text = asm.read_text()
    label = re.search(r"^_ZN5svoxt16fwd_roles_kernelILi1ELi9ELi1ELb1ELb0ELb0E\w*:", text, re.M)
    assert label is not None, "the instance is not in the assembly"
    foot = text[text.index("; Kernel info:", label.end()):][:2000]           # (the footer behind the kernel's code)
    val = {k: int(v) for k, v in re.findall(r"; (NumVgprs|ScratchSize|Occupancy|LDSByteSize): (\d+)", foot)}
    assert set(val) == {"NumVgprs", "ScratchSize", "Occupancy", "LDSByteSize"}, foot[:1500]
    assert val["ScratchSize"] == 0 and val["Occupancy"] == 6 and val["LDSByteSize"] <= 53248 and val["NumVgprs"] <= 80, val
