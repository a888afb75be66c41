"""A host build of the reference's own device code (oracle/_ref/libsvoxt_ref.so) and its ctypes front end.

TEST INFRASTRUCTURE ONLY: imported by tests/test_reference_parity.py, tests/golden/make_reference_golden.py and
__graft_entry__.build(), never by svox_t_amd/.  Building needs the reference tree; a library that was built elsewhere
and travelled with the tree is used as it is where the reference is absent (available(), build()).  The recipe:

  1. read rt_kernel.cu and svox_kernel.cu of the reference (SVOXT_REFERENCE, default /root/reference) and keep each up
     to the end of its device namespace -- everything behind it is the host entry points, whose <<<...>>> launches g++
     cannot parse -- and close the enclosing anonymous namespace.  The two derived files are written to oracle/_ref/,
     which git ignores; they are never committed;
  2. compile oracle/ref_driver.cpp, which includes them, with the stand-in headers of oracle/ref_shim first on the
     include path and the oracle Makefile's numerical flags (-ffp-contract=off -fno-fast-math, no -march);
  3. load the library and mirror oracle.oracle's numpy signatures.

The driver runs every kernel for thread ids 0 .. Q-1 in ascending order on one host thread.
"""
from __future__ import annotations

import ctypes
import os
import subprocess
import sysconfig
from typing import Optional

import numpy as np

from oracle import oracle as O

_HERE = os.path.dirname(os.path.abspath(__file__))
_OUT = os.path.join(_HERE, "_ref")
_LIB_PATH = os.path.join(_OUT, "libsvoxt_ref.so")
_SOURCES = ("rt_kernel", "svox_kernel")
_END_OF_DEVICE_CODE = "}  // namespace device"
CXXFLAGS = ["-O1", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math", "-w"]


def reference_root() -> str:
    return os.environ.get("SVOXT_REFERENCE", "/root/reference")


def _csrc() -> str:
    return os.path.join(reference_root(), "svox_t", "csrc")


def available() -> bool:
    """The library is built, or the reference tree is there to build it from."""
    return os.path.exists(_LIB_PATH) or os.path.isdir(_csrc())


def _derive(name: str) -> str:
    """<name>.cu up to the end of its device namespace, into oracle/_ref/<name>.device.inc."""
    with open(os.path.join(_csrc(), name + ".cu")) as f:
        text = f.read()
    cut = text.find(_END_OF_DEVICE_CODE)
    if cut < 0:
        raise RuntimeError(f"{name}.cu: no '{_END_OF_DEVICE_CODE}' line to cut at")
    cut += len(_END_OF_DEVICE_CODE)
    path = os.path.join(_OUT, name + ".device.inc")
    with open(path, "w") as f:
        f.write(text[:cut] + "\n}  // (anonymous namespace; the host entry points behind it are left out)\n")
    return path


def _inputs():
    shim = os.path.join(_HERE, "ref_shim")
    own = [os.path.join(_HERE, "ref_driver.cpp"), os.path.abspath(__file__)]
    for root, _, files in os.walk(shim):
        own += [os.path.join(root, f) for f in files]
    ref = [os.path.join(_csrc(), n + ".cu") for n in _SOURCES]
    inc = os.path.join(_csrc(), "include")
    if os.path.isdir(inc):
        ref += [os.path.join(inc, f) for f in os.listdir(inc)]
    return own, [p for p in ref if os.path.exists(p)]


def build(force: bool = False) -> str:
    """Compile oracle/_ref/libsvoxt_ref.so when it is missing or older than what it is made from.  Without the reference
    tree an existing library is used as it is."""
    own, ref = _inputs()
    have_ref = os.path.isdir(_csrc())
    if os.path.exists(_LIB_PATH) and not force:
        stamp = os.path.getmtime(_LIB_PATH)
        if not have_ref or all(os.path.getmtime(p) <= stamp for p in own + ref):
            return _LIB_PATH
    if not have_ref:
        raise FileNotFoundError(f"no reference tree at {reference_root()} (set SVOXT_REFERENCE) and no {_LIB_PATH}")
    import torch
    from torch.utils import cpp_extension
    os.makedirs(_OUT, exist_ok=True)
    for name in _SOURCES:
        _derive(name)
    includes = [os.path.join(_HERE, "ref_shim"), _OUT, os.path.join(_csrc(), "include")]
    system = cpp_extension.include_paths() + [sysconfig.get_paths()["include"]]
    libdir = os.path.join(os.path.dirname(torch.__file__), "lib")
    cmd = [os.environ.get("CXX", "g++"), *CXXFLAGS, f"-D_GLIBCXX_USE_CXX11_ABI={int(torch._C._GLIBCXX_USE_CXX11_ABI)}",
           *[f"-I{p}" for p in includes], *[f"-isystem{p}" for p in system],
           "-shared", "-o", _LIB_PATH + ".tmp", os.path.join(_HERE, "ref_driver.cpp"),
           f"-L{libdir}", f"-Wl,-rpath,{libdir}", "-ltorch", "-ltorch_cpu", "-lc10"]
    done = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    if done.returncode != 0:
        raise RuntimeError("building oracle/_ref failed:\n" + " ".join(cmd) + "\n" + done.stdout[-4000:])
    os.replace(_LIB_PATH + ".tmp", _LIB_PATH)
    return _LIB_PATH


class _RefTree(ctypes.Structure):
    """RefTree of oracle/ref_driver.cpp: pointers and int64 only."""
    _fields_ = [(n, t) for n, t in (
        ("features", ctypes.c_void_p), ("M", ctypes.c_int64), ("K", ctypes.c_int64),
        ("data", ctypes.c_void_p), ("child", ctypes.c_void_p), ("parent_depth", ctypes.c_void_p),
        ("n_internal", ctypes.c_int64), ("N", ctypes.c_int64),
        ("offset", ctypes.c_void_p), ("scaling", ctypes.c_void_p),
        ("extra", ctypes.c_void_p), ("extra_rows", ctypes.c_int64), ("extra_cols", ctypes.c_int64),
        ("weight_accum", ctypes.c_void_p),
        ("joint_features", ctypes.c_void_p), ("n_joints", ctypes.c_int64), ("F", ctypes.c_int64),
        ("skinning_weights", ctypes.c_void_p), ("joint_index", ctypes.c_void_p), ("B", ctypes.c_int64),
        ("xform", ctypes.c_void_p), ("xform_rows", ctypes.c_int64), ("xform_dim", ctypes.c_int64))]


_lib = None


def lib():
    global _lib
    if _lib is None:
        build()
        import torch  # noqa: F401  (libtorch is loaded before the library that links it)
        _lib = ctypes.CDLL(_LIB_PATH)
        assert _lib.svoxt_ref_sizeof_options() == ctypes.sizeof(O.RenderOptions)
        assert _lib.svoxt_ref_sizeof_tree() == ctypes.sizeof(_RefTree)
        _lib.svoxt_ref_query_vertical.restype = ctypes.c_int64
    return _lib


def _addr(a: Optional[np.ndarray]):
    return None if a is None else a.ctypes.data


def _p(a: Optional[np.ndarray]):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _c(a, dtype):
    return np.ascontiguousarray(np.asarray(a), dtype=dtype)


def _dbl(dtype) -> int:
    assert dtype in (np.float32, np.float64)
    return int(dtype == np.float64)


def _tree(tree: O.Tree, keep: list, motion: Optional[O.Motion] = None, xform=None, weight_accum=None, parent_depth=None):
    """The C view of an oracle Tree (+ Motion, transformation_matrices [M, d, d], _weight_accum, parent_depth); the arrays
    it points into are appended to `keep`, which the caller holds until the call returns."""
    t = _RefTree()
    t.features, t.M, t.K = _addr(tree.features), tree.M, tree.K
    t.data, t.child, t.n_internal, t.N = _addr(tree.data), _addr(tree.child), tree.child.shape[0], tree.N
    t.offset, t.scaling = _addr(tree.offset), _addr(tree.scaling)
    if tree.extra is not None:
        t.extra, t.extra_rows, t.extra_cols = _addr(tree.extra), tree.extra.shape[0], tree.extra.shape[1]
    if parent_depth is not None:
        pd = _c(parent_depth, np.int32)
        assert pd.shape == (tree.child.shape[0], 2)
        keep.append(pd)
        t.parent_depth = _addr(pd)
    if weight_accum is not None:
        assert weight_accum.dtype == tree.dtype and weight_accum.size == tree.child.size and weight_accum.flags.c_contiguous
        t.weight_accum = _addr(weight_accum)
    if motion is not None:
        assert motion.jf.dtype == tree.dtype and motion.sw.shape[0] == tree.M
        t.joint_features, t.n_joints, t.F = _addr(motion.jf), motion.jf.shape[0], motion.jf.shape[1]
        t.skinning_weights, t.joint_index, t.B = _addr(motion.sw), _addr(motion.ji), motion.ji.shape[1]
    if xform is not None:
        x = _c(xform, tree.dtype)
        assert x.ndim == 3 and x.shape[1] == x.shape[2]
        keep.append(x)
        t.xform, t.xform_rows, t.xform_dim = _addr(x), x.shape[0], x.shape[1]
    return t


def _rays(tree, origins, dirs, vdirs):
    o, d, v = (_c(x, tree.dtype) for x in (origins, dirs, vdirs))
    assert o.shape == d.shape == v.shape and o.shape[1] == 3
    return o, d, v


def volume_render(tree: O.Tree, origins, dirs, vdirs, opt, xform=None, weight_accum=None):
    """render_ray_kernel: [Q, C + 1] of tree.dtype.  weight_accum (tree.dtype, the shape of child) is added to in place."""
    O._check_lobes(opt.format, opt.basis_dim, tree.extra)
    keep = []
    o, d, v = _rays(tree, origins, dirs, vdirs)
    cols = O.out_data_dim(opt, tree.K)
    out = np.empty((o.shape[0], cols), tree.dtype)
    t = _tree(tree, keep, xform=xform, weight_accum=weight_accum)
    lib().svoxt_ref_volume_render(ctypes.byref(t), _dbl(tree.dtype), _p(o), _p(d), _p(v), ctypes.c_int64(o.shape[0]),
                                  ctypes.byref(opt), _p(out), ctypes.c_int64(cols))
    return out


def volume_render_backward(tree: O.Tree, origins, dirs, vdirs, opt, grad_output, xform=None):
    """render_ray_backward_kernel: [M, K] of tree.dtype, the contributions added sequentially in ray order.  With
    grad_output [Q, 1] it is what the reference's opacity_render_backward launches."""
    O._check_lobes(opt.format, opt.basis_dim, tree.extra)
    keep = []
    o, d, v = _rays(tree, origins, dirs, vdirs)
    g = _c(grad_output, tree.dtype)
    assert g.ndim == 2 and g.shape[0] == o.shape[0]
    grad = np.empty((tree.M, tree.K), tree.dtype)
    t = _tree(tree, keep, xform=xform)
    lib().svoxt_ref_volume_render_backward(ctypes.byref(t), _dbl(tree.dtype), _p(o), _p(d), _p(v), ctypes.c_int64(o.shape[0]),
                                           ctypes.byref(opt), _p(g), ctypes.c_int64(g.shape[1]), _p(grad))
    return grad


opacity_render_backward = volume_render_backward


def _cam(tree, c2w):
    c = _c(c2w, tree.dtype)
    assert c.ndim == 2 and c.shape[1] == 4 and c.shape[0] in (3, 4)
    return c


def volume_render_image(tree: O.Tree, c2w, fx, fy, width, height, opt, xform=None):
    """render_image_kernel: [H, W, C + 1]; the NDC warp is taken from opt (ndc_width < 0: none)."""
    O._check_lobes(opt.format, opt.basis_dim, tree.extra)
    keep = []
    c = _cam(tree, c2w)
    cols = O.out_data_dim(opt, tree.K)
    out = np.empty((int(height), int(width), cols), tree.dtype)
    t = _tree(tree, keep, xform=xform)
    lib().svoxt_ref_volume_render_image(ctypes.byref(t), _dbl(tree.dtype), _p(c), ctypes.c_int64(c.shape[0]), ctypes.c_float(fx),
                                        ctypes.c_float(fy), int(width), int(height), ctypes.byref(opt), _p(out), ctypes.c_int64(cols))
    return out


def volume_render_image_backward(tree: O.Tree, c2w, fx, fy, width, height, opt, grad_output, xform=None):
    O._check_lobes(opt.format, opt.basis_dim, tree.extra)
    keep = []
    c = _cam(tree, c2w)
    g = _c(grad_output, tree.dtype)
    assert g.shape[:2] == (int(height), int(width))
    grad = np.empty((tree.M, tree.K), tree.dtype)
    t = _tree(tree, keep, xform=xform)
    lib().svoxt_ref_volume_render_image_backward(ctypes.byref(t), _dbl(tree.dtype), _p(c), ctypes.c_int64(c.shape[0]),
                                                 ctypes.c_float(fx), ctypes.c_float(fy), int(width), int(height), ctypes.byref(opt),
                                                 _p(g), ctypes.c_int64(g.shape[2]), _p(grad))
    return grad


def _per_ray(fn, tree, origins, dirs, vdirs, opt, cols, motion=None):
    keep = []
    o, d, v = _rays(tree, origins, dirs, vdirs)
    out = np.empty((o.shape[0], cols), tree.dtype)
    t = _tree(tree, keep, motion=motion)
    fn(ctypes.byref(t), _dbl(tree.dtype), _p(o), _p(d), _p(v), ctypes.c_int64(o.shape[0]), ctypes.byref(opt), _p(out))
    return out


def opacity_render(tree: O.Tree, origins, dirs, vdirs, opt):
    return _per_ray(lib().svoxt_ref_opacity_render, tree, origins, dirs, vdirs, opt, 1)


def render_depth(tree: O.Tree, origins, dirs, vdirs, opt):
    return _per_ray(lib().svoxt_ref_render_depth, tree, origins, dirs, vdirs, opt, 1)


def motion_feature_render(tree: O.Tree, motion: O.Motion, origins, dirs, vdirs, opt):
    return _per_ray(lib().svoxt_ref_motion_feature_render, tree, origins, dirs, vdirs, opt, motion.jf.shape[1], motion)


def motion_render(tree: O.Tree, origins, dirs, vdirs, opt):
    """-> (joint distances [Q, J], depth [Q, 1], hit_point [Q, 3], data_idx [Q, 1] int64)."""
    assert tree.extra is not None and tree.extra.shape[1] >= 3
    keep = []
    o, d, v = _rays(tree, origins, dirs, vdirs)
    Q, J = o.shape[0], tree.extra.shape[0]
    out, depth, hit = np.empty((Q, J), tree.dtype), np.empty((Q, 1), tree.dtype), np.empty((Q, 3), tree.dtype)
    idx = np.empty((Q, 1), np.int64)
    t = _tree(tree, keep)
    lib().svoxt_ref_motion_render(ctypes.byref(t), _dbl(tree.dtype), _p(o), _p(d), _p(v), ctypes.c_int64(Q), ctypes.byref(opt),
                                  _p(out), _p(depth), _p(hit), _p(idx))
    return out, depth, hit, idx


def grid_weight_render(sigma, c2w, fx, fy, width, height, opt, offset, scaling, dtype=np.float32):
    """grid_weight_render_kernel over the cameras c2w [V, 3 or 4, 4] (or one), one after the other into the same two grids:
    (grid_weight, grid_hit), both of `dtype` and the shape of sigma [R, R, R]."""
    s = _c(sigma, dtype)
    R = s.shape[0]
    assert s.shape[:3] == (R, R, R) and s.size == R ** 3
    cams = _c(c2w, dtype)
    cams = cams[None] if cams.ndim == 2 else cams
    off, sc = _c(offset, dtype), _c(scaling, dtype)
    gw, gh = np.zeros(s.shape, dtype), np.zeros(s.shape, dtype)
    for c in cams:
        c = np.ascontiguousarray(c)
        lib().svoxt_ref_grid_weight_render(_dbl(dtype), _p(s), ctypes.c_int64(R), _p(c), ctypes.c_int64(c.shape[0]), ctypes.c_float(fx),
                                           ctypes.c_float(fy), int(width), int(height), ctypes.byref(opt), _p(off), _p(sc), _p(gw), _p(gh))
    return gw, gh


def query(tree: O.Tree, points):
    """query_vertical's kernels: (values [Q, K], node_ids [Q], data_ids [Q], leaf_node [n_hit, 4]).  The reference
    allocates the first three uninitialised and leaves the rows of points in empty leaves unwritten: here they start
    as 0 / -1, which is what oracle.query writes there."""
    keep = []
    p = _c(points, tree.dtype)
    Q = p.shape[0]
    values = np.zeros((Q, tree.K), tree.dtype)
    node_ids, data_ids = np.full(Q, -1, np.int64), np.full(Q, -1, np.int64)
    leaf = np.zeros((tree.child.size, 4), np.int64)
    t = _tree(tree, keep)
    n = lib().svoxt_ref_query_vertical(ctypes.byref(t), _dbl(tree.dtype), _p(p), ctypes.c_int64(Q), _p(values), _p(node_ids),
                                       _p(data_ids), _p(leaf), ctypes.c_int64(leaf.shape[0]))
    return values, node_ids, data_ids, leaf[:n]


def query_backward(tree: O.Tree, points, grad_output):
    keep = []
    p, g = _c(points, tree.dtype), _c(grad_output, tree.dtype)
    assert g.shape == (p.shape[0], tree.K)
    grad = np.empty((tree.M, tree.K), tree.dtype)
    t = _tree(tree, keep)
    lib().svoxt_ref_query_vertical_backward(ctypes.byref(t), _dbl(tree.dtype), _p(p), ctypes.c_int64(p.shape[0]), _p(g), _p(grad))
    return grad


def warp_vertices(matrices, points, skinning_weights, joint_index, dtype=np.float32):
    """-> (vertices_out [Q, 3], matrix_out [Q, D, D])."""
    m, p, sw, ji = _c(matrices, dtype), _c(points, dtype), _c(skinning_weights, dtype), _c(joint_index, np.int32)
    J, D = m.shape[0], m.shape[1]
    Q, B = sw.shape
    assert m.shape == (J, D, D) and D == 4 and p.shape == (Q, 3) and ji.shape == (Q, B) and ji.min() >= 0 and ji.max() < J
    v, mo = np.empty((Q, 3), dtype), np.empty((Q, D, D), dtype)
    lib().svoxt_ref_warp_vertices(_dbl(dtype), _p(m), ctypes.c_int64(J), ctypes.c_int64(D), _p(p), ctypes.c_int64(Q), _p(sw), _p(ji),
                                  ctypes.c_int64(B), _p(v), _p(mo))
    return v, mo


def warp_vertices_backward(matrices, points, skinning_weights, joint_index, grad_vertices, grad_matrix_out, dtype=np.float32):
    """-> (grad_points [Q, 3], grad_matrices [J, D, D], grad_skinning_weights [Q, B]), all of `dtype`."""
    m, p, sw, ji = _c(matrices, dtype), _c(points, dtype), _c(skinning_weights, dtype), _c(joint_index, np.int32)
    gv, gm = _c(grad_vertices, dtype), _c(grad_matrix_out, dtype)
    J, D = m.shape[0], m.shape[1]
    Q, B = sw.shape
    assert m.shape == (J, D, D) and D == 4 and gv.shape == (Q, 3) and gm.shape == (Q, D, D) and ji.min() >= 0 and ji.max() < J
    gp, gmat, gsw = np.empty((Q, 3), dtype), np.empty((J, D, D), dtype), np.empty((Q, B), dtype)
    lib().svoxt_ref_warp_vertices_backward(_dbl(dtype), _p(m), ctypes.c_int64(J), ctypes.c_int64(D), _p(p), ctypes.c_int64(Q), _p(sw),
                                           _p(ji), ctypes.c_int64(B), _p(gv), _p(gm), _p(gp), _p(gmat), _p(gsw))
    return gp, gmat, gsw


def calc_corners(tree: O.Tree, parent_depth, leaf_node):
    """calc_corner_kernel: [Q, 3] of tree.dtype, the lower corner in [0, 1)^3 of every leaf slot (node, u, v, w)."""
    keep = []
    ix = _c(leaf_node, np.int64)
    assert ix.ndim == 2 and ix.shape[1] == 4
    out = np.empty((ix.shape[0], 3), tree.dtype)
    t = _tree(tree, keep, parent_depth=parent_depth)
    lib().svoxt_ref_calc_corners(ctypes.byref(t), _dbl(tree.dtype), _p(ix), ctypes.c_int64(ix.shape[0]), _p(out))
    return out
