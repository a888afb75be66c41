"""The per-sample interface: march -> samples -> weights from density -> accumulate along rays.

    samples = renderer.ray_samples(rays, min_sigma=0.0)            # RaySamples: CSR lists of the leaf crossings
    f = gather_rows(samples, features)                             # [T, K]: the feature row of every sample
    w, alpha = sample_weights(samples, f[:, -1])                   # w_k = T_k (1 - exp(-length_k sigma_k)), alpha = 1 - T_end
    out = accumulate(samples, w, values)                           # out[q] = sum_k w_k values_k over ray q's samples
    out, alpha, w = composite(samples, f[:, -1], values)           # the two chained
    wmax = reduce_rows(samples, w.detach(), M, "max")              # [M]: a per-row statistic of per-sample values
    rgb, sigma = renderer.shade_samples(samples, features, rays)   # [T, C], [T]: the samples' colours and densities, no [T, K]
                                                                   # (differentiable in features, and in rays.viewdirs / basis: DESIGN.md 4.30)
    rgb, sigma = renderer.shade_samples(samples, features, rays, rotations=mats)   # the basis at mats[row] @ viewdirs[ray], what forward's
                                                                   # transformation_matrices do; differentiable in mats too
    trans = ray_scan(samples, att, "prod", exclusive=True)         # running sum / prod / max / min along every ray
    index, frac = ray_quantile(samples, w, [0.5])                  # where the running weight crosses q * total; quantile_depth: the depth
    sub, index = samples.select(w > 1e-3)                          # the kept samples as a RaySamples of its own; values[index] follows
    fine, index = samples.split(max_length=0.01)                   # every crossing cut into equal pieces (or pieces=int32 [T])
    m, ia, ib = merge_samples(sa, sb)                              # two trees a ray: the union of two lists of the SAME rays, and
    s_a, s_b = take_samples(sig_a, ia), take_samples(sig_b, ib)    # per piece each list's sample or -1: 0 where a tree has no sample there
    samples = renderer.ray_samples(rays, faces=True)               # + samples.face: the planes every crossing begins and ends on, and
    depth, length = sample_geometry(samples, rays)                 # the two list arrays, differentiable in rays.origins / rays.dirs
    w, alpha = sample_weights(samples, sigma, length=length)       # (a camera pose refined against a fixed tree)

Every per-sample loss is then a few lines of torch around HIP operators whose results, gradients included, have the same
bits in every run: the gradient of gather_rows reaches the table through reduce_rows' fixed-order row plan (DESIGN.md
4.21), not through float atomics.  There is no CPU path.
"""
from __future__ import annotations

import torch
from torch import autograd

from svox_t_amd.helpers import _get_c_extension
from svox_t_amd.renderer import Rays, VolumeRenderer, _rays_spec_from_rays

_C = _get_c_extension()
_X = _C._extras            # (ray_scan / ray_quantile / select's wrappers are reached here, not as csrc.* names)


class RaySamples:
    """The leaf crossings of a ray batch in CSR form, in ray-index order and, within a ray, in march order.

    offsets int64 [Q + 1]   ray q's samples are offsets[q] .. offsets[q + 1] - 1
    ray     int32 [T]       the ray of every sample
    row     int32 [T]       the feature row of the leaf crossed
    depth   float32 [T]     distance at which the ray enters the leaf (the "entry" z of render_depth_moments)
    length  float32 [T]     length of the crossing (+ step_size), in the same units
    face    uint8 [T]       optional (ray_samples(faces=True), else None): entry | exit << 2, the axis (0, 1, 2) of the plane
                            the crossing begins on -- 3: none, the ray starts inside the cube -- and of the one it ends on
                            (include/svoxt.h, svoxt_ray_samples_emit_faces); what sample_geometry needs
    """

    def __init__(self, offsets, ray, row, depth, length, face=None):
        self.offsets, self.ray, self.row, self.depth, self.length, self.face = offsets, ray, row, depth, length, face
        if not isinstance(offsets, torch.Tensor) or offsets.dtype != torch.int64 or offsets.dim() != 1 or offsets.shape[0] < 1:
            raise RuntimeError("offsets must be int64 [Q + 1]")
        T = ray.shape[0] if isinstance(ray, torch.Tensor) and ray.dim() == 1 else -1
        for name, x, dt in (("ray", ray, torch.int32), ("row", row, torch.int32), ("depth", depth, torch.float32),
                            ("length", length, torch.float32)):
            if not isinstance(x, torch.Tensor) or x.dtype != dt or tuple(x.shape) != (T,):
                raise RuntimeError(f"{name} must be {str(dt).split('.')[-1]} [T], one entry per sample")
        if face is not None:
            if not isinstance(face, torch.Tensor) or face.dtype != torch.uint8 or tuple(face.shape) != (T,):
                raise RuntimeError("face must be uint8 [T], one entry per sample")
            if face.device != ray.device:
                raise RuntimeError("face must be on the device of the samples")

    @property
    def Q(self) -> int:
        return self.offsets.shape[0] - 1

    def __len__(self) -> int:
        return self.ray.shape[0]

    @property
    def counts(self):
        """int64 [Q]: the number of samples of every ray."""
        return self.offsets[1:] - self.offsets[:-1]

    def row_plan(self, M: int) -> "RowPlan":
        """The RowPlan of these lists for a feature table of M rows: for every row the samples that name it, in
        ascending sample index.  Built on the GPU with one host read and cached on this object per M: the tensors of
        a RaySamples are not meant to be edited -- a plan built before an edit of `row` describes the old rows."""
        M = _C._extras._check_rows_extent(M, "row_plan")
        if not self.row.is_cuda:
            raise RuntimeError("row_plan: only the GPU (HIP) path exists; the samples must be on the GPU")
        plans = self.__dict__.setdefault("_row_plans", {})
        if M not in plans:
            arrays = _C.row_plan(self.row.contiguous(), M)
            plans[M] = _C._Produced("row_plan", RowPlan(arrays), arrays, self.row.device)
        return plans[M].ready_on(_C._raw_stream(self.row.device))    # (built on another stream: that stream waits for it)

    def points(self, rays: Rays, at: str = "mid", *, geometry=None):
        """float32 [T, 3]: a world point per sample, origins[ray] + dirs[ray] * z with z = depth + 0.5 * length ("mid") or
        z = depth ("entry") -- what tree.interp(samples.points(rays)) looks up in front of sample_weights / accumulate.
        `rays` are the Rays the samples were marched from, with explicit origins and dirs; depth is measured along
        `dirs` as given (the march's own scale).  Plain torch, differentiable in nothing.  Camera-mode and NDC rays are
        refused: their origins and directions are formed inside the kernels.

        :param geometry: (depth, length), two float32 [T] tensors -- sample_geometry(samples, rays)'s -- used in place of
            the lists' own: the same formula without no_grad, differentiable in rays.origins, rays.dirs and both tensors."""
        if at not in ("mid", "entry"):
            raise RuntimeError('points: at must be "mid" or "entry"')
        if not isinstance(rays, Rays):
            raise RuntimeError("points: rays must be the Rays the samples were marched from (camera-mode and NDC rays are "
                               "not served: their origins and directions are formed inside the kernels)")
        o, d = rays.origins, rays.dirs
        for name, x in (("origins", o), ("dirs", d)):
            if not isinstance(x, torch.Tensor) or x.dtype != torch.float32 or tuple(x.shape) != (self.Q, 3):
                raise RuntimeError(f"points: rays.{name} must be float32 [Q, 3] with Q = {self.Q}, the rays the samples were marched from")
            if x.device != self.ray.device:
                raise RuntimeError("points: the rays must be on the device of the samples")
        if geometry is not None:
            if not isinstance(geometry, (tuple, list)) or len(geometry) != 2:
                raise RuntimeError("points: geometry must be (depth, length), as sample_geometry returns them")
            for name, x in zip(("depth", "length"), geometry):
                if not isinstance(x, torch.Tensor) or x.dtype != torch.float32 or tuple(x.shape) != (len(self),) or x.device != self.ray.device:
                    raise RuntimeError(f"points: geometry's {name} must be float32 [T] on the device of the samples")
            depth, length = geometry
            z = depth + 0.5 * length if at == "mid" else depth
            idx = self.ray.long()
            return o[idx] + d[idx] * z[:, None]
        with torch.no_grad():
            z = self.depth + 0.5 * self.length if at == "mid" else self.depth
            idx = self.ray.long()
            return o.detach()[idx] + d.detach()[idx] * z[:, None]

    def select(self, keep):
        """(RaySamples, index int64 [T']): the samples with keep[k] set, in their old order, as lists of their own -- the
        same Q rays (a ray may become empty), ray / row / depth / length copied bit for bit -- and every kept sample's
        position in the old lists: values[index] carries any per-sample tensor over, gradients flow through torch's
        indexing.  `face` is carried where the lists have it.  `keep` is torch.bool [T] on the samples' device.  Flag, scan, emit on the GPU with one host read (T');
        the result holds no cached row plan."""
        if not isinstance(keep, torch.Tensor) or keep.dtype != torch.bool or tuple(keep.shape) != (len(self),):
            raise RuntimeError("select: keep must be torch.bool [T], one entry per sample")
        _require_gpu("select", self, keep)
        with torch.no_grad():
            offsets, ray, row, depth, length, index, _ = _X.samples_select(
                keep.contiguous(), self.offsets.contiguous(), self.ray.contiguous(), self.row.contiguous(), self.depth.contiguous(),
                self.length.contiguous())
            face = None if self.face is None else self.face[index]
        return RaySamples(offsets, ray, row, depth, length, face), index

    def split(self, max_length=None, *, pieces=None, max_pieces: int = 4096):
        """(RaySamples, index int64 [T']): every sample cut into equal pieces, in list order, as lists of their own over
        the same Q rays, and every piece's source sample: values[index] carries any per-sample tensor over.  Exactly one
        of `max_length` (a Python float > 0, inf allowed: no piece longer than it) and `pieces` (int32 [T] on the samples'
        device: a count per sample).  For sample k, float32, every operation rounded by itself:

            mf = ceilf(length / max_length)  or  (float)pieces[k]
            m = 1 where length > 0 is false (0, negative, NaN) or mf >= 1 is false;  else m = (int)min(mf, (float)max_pieces)
            m == 1: the sample copied bit for bit;  else step = length / (float)m, piece p: depth + (float)p * step, length step

        Every piece keeps `ray` and `row`.  split(max_length=inf) and split(pieces=ones) are these lists array for array.
        Count, scan, emit on the GPU -- a lane per OUTPUT piece, which finds its source by a binary search in the scan --
        with one host read (T'); a result of 2^31 samples or more is refused before anything is allocated.  Not
        differentiable: the results are indices and distances.  The result holds no cached row plan and no `face`: a piece's
        ends are not leaf faces (sample_geometry refuses it; carry depth[index], length[index] over in torch instead)."""
        if (max_length is None) == (pieces is None):
            raise RuntimeError("split: exactly one of max_length and pieces must be given")
        if pieces is not None and (not isinstance(pieces, torch.Tensor) or pieces.dtype != torch.int32 or tuple(pieces.shape) != (len(self),)):
            raise RuntimeError("split: pieces must be int32 [T], one entry per sample")
        if pieces is None and (isinstance(max_length, (bool, torch.Tensor)) or not isinstance(max_length, (int, float)) or not max_length > 0):
            raise RuntimeError("split: max_length must be a float > 0 (inf allowed)")
        if isinstance(max_pieces, bool) or not isinstance(max_pieces, int) or not 1 <= max_pieces <= _X.SPLIT_MAX_PIECES:
            raise RuntimeError("split: max_pieces must be an int in [1, 2^30]")
        _require_gpu("split", self, pieces)
        with torch.no_grad():
            offsets, ray, row, depth, length, index, _ = _X.samples_split(
                self.offsets.contiguous(), self.ray.contiguous(), self.row.contiguous(), self.depth.contiguous(), self.length.contiguous(),
                max_length, None if pieces is None else pieces.contiguous(), max_pieces)
        return RaySamples(offsets, ray, row, depth, length), index


def merge_samples(a: RaySamples, b: RaySamples):
    """(RaySamples m, index_a int64 [T'], index_b int64 [T']): the union of two lists along shared rays -- per ray the
    pieces between all breakpoints of both lists that at least one of them covers, and for every piece the sample of `a`
    and of `b` that covers it (-1: none): take_samples(values_a, index_a) carries a per-sample tensor of `a` over.

    `a` and `b` must be lists of the SAME rays -- the same Q, the same origins and direction vectors, as from two
    renderers' ray_samples(rays) -- through two trees of any centre and radius: `depth` is the parameter along `dirs` as
    given (RaySamples.points), so the depths of both lists are comparable.  Only Q and the device are checked.  m.row is -1
    everywhere: a merged sample names no single feature row; rows are reached through gather_rows(a, table_a) and
    take_samples(..., index_a).  m holds no cached row plan.

    The walk (include/svoxt.h states it rule by rule): a sample is [s, e) with s = depth, e = depth + length (one float32
    add); neighbours inside one list are never compared.  A sample with e > s false (length 0, negative or NaN, NaN depth)
    is emitted whole and alone, A's before B's, and cuts nothing.  Otherwise the pieces run from breakpoint to breakpoint;
    a piece that is all of a source sample takes that sample's length bit for bit, any other the float32 difference of
    its ends.  So merge_samples(a, empty) is `a` array for array with index_a = arange and index_b = -1 (mirrored for b);
    merge_samples(a, a) is `a` with both indices arange where no sample of `a` is degenerate; a ray has at most
    2 (n_a + n_b) pieces; the pieces with index_a == k tile [s_k, e_k).  Output depths are monotone except where an input
    list overlaps itself: the march's own neighbours overlap by a unit in the last place now and then, and the sliver is
    emitted as a piece.  With sigma = sigma_a + sigma_b per piece the composite of two piecewise-constant media is exact
    in the sense of the interval form.

    A lane per ray walks both segments, once to count and once to emit; one host read (T'), refused from 2^31 on before
    anything is allocated.  Not differentiable: indices and distances; m.face is None (see split).  There is no CPU path."""
    if not isinstance(a, RaySamples) or not isinstance(b, RaySamples):
        raise RuntimeError("merge_samples: a and b must be RaySamples")
    if a.Q != b.Q:
        raise RuntimeError(f"merge_samples: a holds {a.Q} rays, b {b.Q}; they must be lists of the same rays")
    _require_gpu("merge_samples", a)
    _require_gpu("merge_samples", b)
    if a.offsets.device != b.offsets.device:
        raise RuntimeError("merge_samples: a and b must be on the same device")
    with torch.no_grad():
        offsets, ray, row, depth, length, index_a, index_b, _ = _X.samples_merge(
            a.offsets.contiguous(), a.depth.contiguous(), a.length.contiguous(), b.offsets.contiguous(), b.depth.contiguous(),
            b.length.contiguous())
    return RaySamples(offsets, ray, row, depth, length), index_a, index_b


def take_samples(values, index, fill: float = 0.0):
    """values[index] where index >= 0 and `fill` where it is -1 (merge_samples: the piece has no sample of that list);
    -1 never wraps to the last element.  values: [T, ...], index: int64 [T']; the result is [T', ...].  Plain torch:
    gradients reach `values` through the indexing."""
    if not isinstance(values, torch.Tensor) or values.dim() < 1:
        raise RuntimeError("take_samples: values must be a tensor [T, ...], one row per sample")
    if not isinstance(index, torch.Tensor) or index.dtype != torch.int64 or index.dim() != 1:
        raise RuntimeError("take_samples: index must be int64 [T']")
    if values.shape[0] == 0:
        return values.new_full((index.shape[0],) + tuple(values.shape[1:]), fill)
    hit = index >= 0
    out = values[index.clamp_min(0)]
    return torch.where(hit.reshape((-1,) + (1,) * (values.dim() - 1)), out, torch.full_like(out, fill))


class RowPlan:
    """The inverse of a RaySamples' `row` list for a table of M rows (include/svoxt.h, "the row plan").

    row_ptr   int32 [M + 1]   row r's samples are perm[row_ptr[r]] .. perm[row_ptr[r + 1] - 1], in ascending sample index
    perm      int32 [T]       the sample indices sorted stably by key: `row` where 0 <= row < M, M for anything else
    n_outside, longest        the samples whose row lies outside [0, M) (they sort behind row_ptr[M] and take no part in
                              anything), and the length of the longest segment
    Rows of more than 256 samples are listed (long_rows, long_chunk_ptr, chunk_long): reduce_rows sums them in chunks."""

    def __init__(self, arrays):
        self.arrays = arrays
        self.row_ptr, self.perm, self.M, self.T = arrays.row_ptr, arrays.perm, arrays.M, arrays.T
        self.n_outside, self.longest = arrays.n_outside, arrays.longest
        self.long_rows, self.long_chunk_ptr, self.chunk_long = arrays.long_rows, arrays.long_chunk_ptr, arrays.chunk_long

    @property
    def counts(self):
        """int32 [M]: the number of samples of every row."""
        return self.row_ptr[1:] - self.row_ptr[:-1]


def _ray_samples(self, rays: Rays, *, features=None, min_sigma=None, image_shape=None, sort_rays=None, faces=False) -> RaySamples:
    """The leaf crossings of a ray batch as RaySamples: every crossing of the shared march whose leaf holds a feature
    row, or with `min_sigma` only those whose sigma exceeds it (0.0: the set the backwards walk, sigma > 0).

    :param features: the feature table sigma is read from (default: the tree's own); read only with min_sigma
    :param image_shape, sort_rays: see forward -- they change how the rays are walked, never the lists
    :param faces: also fill RaySamples.face, a byte per sample (entry | exit << 2: the axes of the planes the crossing
        begins and ends on); the other five arrays are those of faces=False bit for bit.  The emit kernel is another one.
    Nothing here is differentiable: the lists are indices and distances of the march; sample_geometry(samples, rays) of a
    faces=True list is the route from depth and length back to rays.origins and rays.dirs.  One host read (the total)."""
    self._require_gpu(True, "ray_samples")
    if features is None:
        features = self.tree.features
    with torch.no_grad():
        spec = self.tree._spec(features.detach())
        rspec = _rays_spec_from_rays(rays, image_shape, sort_rays)
        rspec.need_grad = False
        if not faces:
            offsets, row, ray, depth, length, _ = _C.ray_samples(spec, rspec, self._get_options(), min_sigma)
            return RaySamples(offsets, ray, row, depth, length)
        offsets, row, ray, depth, length, _, face = _C.ray_samples(spec, rspec, self._get_options(), min_sigma, True)
    return RaySamples(offsets, ray, row, depth, length, face)


VolumeRenderer.ray_samples = _ray_samples


# ------------------------------------------------------------------------------------------------ shading the samples
def _refuse_transformation_matrices(what):
    raise RuntimeError(f"VolumeRenderer.{what}: transformation_matrices are not served: the per-leaf rotation of the view "
                       "direction is out of scope here (forward takes them; shade_samples takes them as `rotations=`, with "
                       "`rays=`; see INTEGRATION.md)")


class _ViewBasisFunction(autograd.Function):
    @staticmethod
    def forward(ctx, viewdirs, renderer, rays, image_shape):
        basis = _C.view_basis(renderer.tree._spec(renderer.tree.features.detach()), _rays_spec_from_rays(rays, image_shape),
                              renderer._get_options())
        ctx.renderer, ctx.rays = renderer, rays
        ctx.save_for_backward(basis)
        return basis

    @staticmethod
    @autograd.function.once_differentiable
    def backward(ctx, grad_basis):
        (basis,) = ctx.saved_tensors
        r, rays = ctx.renderer, ctx.rays
        with torch.no_grad():
            spec = _rays_spec_from_rays(Rays(rays.origins.detach(), rays.dirs.detach(), rays.viewdirs.detach()))
            spec.need_grad = False
            gv = _X.view_basis_backward(r.tree._spec(r.tree.features.detach()), spec, r._get_options(), basis, grad_basis.contiguous())
        return gv, None, None, None


def _view_basis(self, rays: Rays, *, image_shape=None, transformation_matrices=None):
    """basis float32 [Q, basis_dim]: every ray's basis values exactly as the render kernels form them from its view
    direction -- SH 1 / 4 / 9 / 16 / 25, SG / ASG from tree.extra_data -- every component, whatever [min_comp, max_comp]
    says.  RGBA: an empty [Q, 0] tensor.  A lane per ray, no march.  `image_shape` is accepted as the neighbours take it
    and changes nothing.

    Differentiable in rays.viewdirs when `rays` is an explicit Rays whose viewdirs require grad (the same forward, the
    same bits): the backward is one kernel, a lane per ray, the analytic derivative of the expression the forward
    evaluates summed over the components in ascending order (include/svoxt.h, svoxt_view_basis_bwd, is the definition;
    DESIGN.md 4.30).  The derivative is taken in the three components as given -- the forward does not normalise, so
    nothing is projected on the sphere; pinhole_rays' own normalisation is torch and supplies the rest of the chain.  Once
    differentiable; not in the SG / ASG lobe parameters.  Every other call runs under no_grad as before."""
    if transformation_matrices is not None:
        _refuse_transformation_matrices("view_basis")
    self._require_gpu(True, "view_basis")
    if isinstance(rays, Rays) and isinstance(rays.viewdirs, torch.Tensor) and rays.viewdirs.requires_grad and torch.is_grad_enabled() \
            and int(self._get_options().format) != 0:
        return _ViewBasisFunction.apply(rays.viewdirs, self, rays, image_shape)
    with torch.no_grad():
        return _C.view_basis(self.tree._spec(self.tree.features.detach()), _rays_spec_from_rays(rays, image_shape), self._get_options())


def _upstream(g):
    """An upstream gradient as the kernels take it: contiguous, or None (zeros: the kernel's null pointer)."""
    return None if g is None else g.contiguous()


class _ShadeSamplesFunction(autograd.Function):
    @staticmethod
    def forward(ctx, features, samples, basis, opt, activate):
        features = features.contiguous()
        basis_grad = basis is not None and basis.requires_grad
        if basis is not None:
            basis = basis.detach().contiguous()
        values, sigma = _C.shade_samples_fwd(features, samples.row, samples.ray, basis, samples.Q, opt, activate)
        ctx.samples, ctx.opt, ctx.activate, ctx.shape = samples, opt, activate, tuple(features.shape)
        ctx.has_basis, ctx.basis_grad = basis is not None, basis_grad
        ctx.set_materialize_grads(False)                         # (a None upstream gradient stays None: the kernel's null pointer)
        saved = (values,) if basis is None else (values, basis)  # (sig: the forward's own output)
        ctx.save_for_backward(*(saved + (features,) if basis_grad else saved))      # (the table: only for grad_basis)
        return values, sigma

    @staticmethod
    def backward(ctx, grad_values, grad_sigma):
        need_basis = ctx.basis_grad and ctx.needs_input_grad[2]
        if need_basis and torch.is_grad_enabled():
            raise RuntimeError("shade_samples: the gradient in `basis` is once differentiable (no double backward)")
        if not (ctx.needs_input_grad[0] or need_basis):
            return None, None, None, None, None
        values = ctx.saved_tensors[0]
        basis = ctx.saved_tensors[1] if ctx.has_basis else None
        s = ctx.samples
        gv, gs = _upstream(grad_values), _upstream(grad_sigma)
        grad = grad_basis = None
        if ctx.needs_input_grad[0]:
            plan = s.row_plan(ctx.shape[0])
            grad = _C.shade_samples_bwd(ctx.shape, s.ray, basis, s.Q, ctx.opt, ctx.activate, values, gv, gs, plan.arrays)
        if need_basis:
            grad_basis = _X.shade_samples_bwd_basis(ctx.saved_tensors[2], s.offsets.contiguous(), s.row, s.ray, s.Q, ctx.opt, ctx.activate,
                                                    values, gv)
        return grad, None, grad_basis, None, None


class _ShadeRotatedFunction(autograd.Function):
    """shade_samples(rotations=): the rotated call's own Function; the plain call keeps _ShadeSamplesFunction."""

    @staticmethod
    def forward(ctx, features, rotations, viewdirs, samples, extra, opt, activate):
        features, rotations, viewdirs = features.contiguous(), rotations.contiguous(), viewdirs.contiguous()
        values, sigma = _X.shade_rot_fwd(features, samples.row, samples.ray, rotations, viewdirs, extra, samples.Q, opt, activate)
        ctx.samples, ctx.extra, ctx.opt, ctx.activate = samples, extra, opt, activate
        ctx.view_grad = ctx.needs_input_grad[1] or ctx.needs_input_grad[2]
        ctx.set_materialize_grads(False)                         # (a None upstream gradient stays None: the kernel's null pointer)
        ctx.shape = tuple(features.shape)
        saved = (values, viewdirs, rotations)                    # (sig: the forward's own output)
        ctx.save_for_backward(*(saved + (features,) if ctx.view_grad else saved))      # (the table: only for gu)
        return values, sigma

    @staticmethod
    def backward(ctx, grad_values, grad_sigma):
        need_f, need_r, need_v = ctx.needs_input_grad[:3]
        if not (need_f or need_r or need_v):
            return (None,) * 7
        if torch.is_grad_enabled():
            raise RuntimeError("shade_samples: the gradients of the rotated call are once differentiable (no double backward)")
        values, viewdirs, rotations = ctx.saved_tensors[:3]
        s, M = ctx.samples, ctx.shape[0]
        gv, gs = _upstream(grad_values), _upstream(grad_sigma)
        grad = grad_rot = grad_view = None
        if need_f:
            grad = _X.shade_rot_bwd(ctx.shape, s.row, s.ray, rotations, viewdirs, ctx.extra, s.Q, ctx.opt, ctx.activate, values, gv, gs,
                                    s.row_plan(M).arrays)
        if need_r or need_v:
            gu = _X.shade_rot_bwd_dir(ctx.saved_tensors[3], s.row, s.ray, rotations, viewdirs, ctx.extra, s.Q, ctx.opt, ctx.activate,
                                      values, gv)
            if need_r:
                grad_rot = _X.shade_rot_bwd_rotations(gu, viewdirs, s.ray, tuple(rotations.shape), s.row_plan(M).arrays)
            if need_v:
                grad_view = _X.shade_rot_bwd_viewdirs(gu, rotations, s.offsets.contiguous(), s.row, s.ray)
        return grad, grad_rot, grad_view, None, None, None, None


def _shade_rotated(self, samples, features, rays, rotations, opt, activate):
    """shade_samples(rotations=) for a format with a basis: the checks of the view side, then the rotated Function."""
    if not isinstance(rays, Rays):
        raise RuntimeError("shade_samples: `rotations` needs `rays`, the Rays the samples were marched from, with explicit viewdirs "
                           "(camera-mode and NDC rays are not served: their directions are formed inside the kernels)")
    v = rays.viewdirs
    if not isinstance(v, torch.Tensor) or v.dtype != torch.float32 or tuple(v.shape) != (samples.Q, 3):
        raise RuntimeError(f"shade_samples: rays.viewdirs must be float32 [Q, 3] with Q = {samples.Q}, the rays the samples were marched from")
    if v.device != features.device:
        raise RuntimeError("shade_samples: the rays must be on the device of the features")
    self._require_gpu(True, "shade_samples")
    _require_gpu("shade_samples", samples, features, rotations, v)
    extra = None
    if int(opt.format) in (2, 3):                                # SG / ASG: the lobes
        extra = self.tree.extra_data
        extra = None if extra is None else extra.detach().contiguous()
    return _ShadeRotatedFunction.apply(features, rotations, v, samples, extra, opt, activate)


def _shade_samples(self, samples: RaySamples, features=None, rays: Rays = None, *, basis=None, activate=True,
                   transformation_matrices=None, rotations=None):
    """(values float32 [T, C], sigma float32 [T]): the colour of every sample -- the basis of its ray's view direction
    dotted into its feature row's coefficients over [min_comp, max_comp], then the sigmoid (activate=False: the dot
    product itself) -- and its density features[row, -1].  C = out_data_dim - 1: K - 1 for RGBA, (K - 1) // basis_dim
    otherwise.  The arithmetic is the render kernels', operation for operation (include/svoxt.h,
    svoxt_shade_samples_fwd).  A sample whose row is outside [0, M) gets zeros and no gradient.

    :param features: float32 [M, K] (default: the tree's own)
    :param rays: the Rays the samples were marched from (view_basis is called), or
    :param basis: what view_basis returned for them, float32 [Q, basis_dim]; RGBA needs neither
    Differentiable in `features`: the gradient is a full [M, K] table, every element written, summed per entry over
    samples.row_plan(M) in reduce_rows' fixed order -- no [T, K] tensor, no atomics, the same bits in every run.

    Differentiable in `basis` too where it requires grad (and through `rays=` in rays.viewdirs: view_basis is then the
    differentiable call): grad_basis[q, i] = the sum over ray q's samples in list order, and over c ascending inside a
    sample, of (grad_values[k, c] * d[k, c]) * features[row[k], c * basis_dim + i], d the factor the table's gradient uses
    (include/svoxt.h, svoxt_shade_samples_bwd_basis, is the definition).  basis_dim lanes a ray walk its
    segment together; exact zeros outside [min_comp, max_comp] and for a ray without samples; no atomics, no [T, K]
    tensor.  Each gradient is computed only when asked for; `features` is kept for the backward only when the basis
    requires grad.  Once differentiable.

    :param rotations: float32 [M, 3, 3] or [M, 4, 4] (the upper-left 3 x 3 is read), one matrix per FEATURE ROW, indexed as
        forward(transformation_matrices=) indexes it -- what warp_vertices(...)[1] or blend_transformation_matrix
        returns: the basis is evaluated at u = rotations[row[k]] @ viewdirs[ray[k]] for every sample, nothing normalised
        (include/svoxt.h, svoxt_shade_rot_fwd, is the definition).  Needs `rays`, an explicit Rays;
        excludes `basis`.  RGBA ignores it, as forward does.  A Function of its own, differentiable once in `features`
        (the same full [M, K] table over the row plan, the basis values recomputed from the matrix and the direction),
        in `rotations` (grad[m, a, b] = the sum over the row plan, in reduce_rows' order, of gu[k, a] * viewdirs[ray[k], b])
        and in rays.viewdirs (per ray in list order, acc[b] += rotations[row[k], a, b] * gu[k, a]); gu float32 [T, 3], 12
        bytes a sample, is view_basis' backward at u with grad_basis[i] = sum_c (grad_values[k, c] * d[k, c]) *
        features[row[k], c * basis_dim + i].  No atomics, the same bits in every run; each gradient only when asked for;
        `features` is kept for the backward only when rotations or viewdirs require grad.  Without `rotations` nothing
        changes.  The keyword `transformation_matrices` stays refused here and on view_basis (a per-ray basis has no row)."""
    if transformation_matrices is not None:
        _refuse_transformation_matrices("shade_samples")
    if not isinstance(samples, RaySamples):
        raise RuntimeError("shade_samples: samples must be a RaySamples")
    if features is None:
        features = self.tree.features
    if not isinstance(features, torch.Tensor) or features.dtype != torch.float32 or features.dim() != 2 or features.shape[1] < 1:
        raise RuntimeError("shade_samples: features must be float32 [M, K], K >= 1")
    opt = self._get_options()
    if rotations is not None:
        if basis is not None:
            raise RuntimeError("shade_samples: `rotations` and `basis` exclude each other: a per-ray basis has no row to rotate by "
                               "(pass `rays`)")
        if not _X._is_rotations(rotations):
            raise RuntimeError("shade_samples: rotations must be float32 [M, 3, 3] or [M, 4, 4], one matrix per feature row")
        if rotations.shape[0] != features.shape[0]:
            raise RuntimeError(f"shade_samples: rotations holds {rotations.shape[0]} matrices, the feature table {features.shape[0]} rows")
        if rotations.device != features.device:
            raise RuntimeError("shade_samples: rotations must be on the device of the features")
        if int(opt.format) != 0:
            return _shade_rotated(self, samples, features, rays, rotations, opt, bool(activate))
    if int(opt.format) == 0:
        basis = None                                             # (RGBA: no basis, and rotations rotate nothing -- uses_xform)
    elif basis is None:
        if rays is None:
            raise RuntimeError("shade_samples: a format with a basis needs `rays` or a `basis` from view_basis")
    elif not isinstance(basis, torch.Tensor) or basis.dtype != torch.float32 or tuple(basis.shape) != (samples.Q, int(opt.basis_dim)):
        raise RuntimeError(f"shade_samples: basis must be float32 [Q, basis_dim] = [{samples.Q}, {int(opt.basis_dim)}], "
                           "view_basis of the samples' rays")
    self._require_gpu(True, "shade_samples")
    _require_gpu("shade_samples", samples, features, basis)
    if int(opt.format) != 0:
        if basis is None:
            basis = self.view_basis(rays)                        # (differentiable where rays.viewdirs requires grad)
        elif not (basis.requires_grad and torch.is_grad_enabled()):
            basis = basis.detach().contiguous()
        if basis.shape[0] != samples.Q:
            raise RuntimeError(f"shade_samples: `rays` holds {basis.shape[0]} rays, the samples were marched from {samples.Q}")
    return _ShadeSamplesFunction.apply(features, samples, basis, opt, bool(activate))


VolumeRenderer.view_basis = _view_basis
VolumeRenderer.shade_samples = _shade_samples


def shade_samples(renderer: VolumeRenderer, samples: RaySamples, features=None, rays: Rays = None, *, basis=None, activate=True,
                  rotations=None):
    """renderer.shade_samples(samples, features, rays, basis=basis, activate=activate, rotations=rotations) as a function,
    beside gather_rows."""
    if not isinstance(renderer, VolumeRenderer):
        raise RuntimeError("shade_samples: the first argument must be the VolumeRenderer whose format shades the samples")
    return renderer.shade_samples(samples, features, rays, basis=basis, activate=activate, rotations=rotations)


def _require_gpu(what, samples, *tensors):
    if not isinstance(samples, RaySamples):
        raise RuntimeError(f"{what}: samples must be a RaySamples")
    for x in (samples.offsets,) + tensors:
        if x is not None and not x.is_cuda:
            raise RuntimeError(f"{what}: only the GPU (HIP) path exists; the samples and every argument must be on the GPU")


class _SampleWeightsFunction(autograd.Function):
    @staticmethod
    def forward(ctx, sigma, samples, length=None):
        sigma = sigma.contiguous()
        ctx.has_length = length is not None
        length = samples.length if length is None else length.contiguous()
        w, alpha = _C.sample_weights(samples.offsets, length, sigma)
        ctx.samples = samples
        ctx.save_for_backward(*((sigma, length) if ctx.has_length else (sigma,)))
        return w, alpha

    @staticmethod
    def backward(ctx, grad_w, grad_alpha):
        need_length = ctx.has_length and ctx.needs_input_grad[2]
        if not (ctx.needs_input_grad[0] or need_length):
            return None, None, None
        sigma = ctx.saved_tensors[0]
        s = ctx.samples
        length = ctx.saved_tensors[1] if ctx.has_length else s.length
        gw = None if grad_w is None else grad_w.contiguous()
        ga = None if grad_alpha is None else grad_alpha.contiguous()
        if not need_length:
            return _C.sample_weights_backward(s.offsets, length, sigma, gw, ga), None, None
        gs, gl = _X.sample_weights_backward_length(s.offsets, length, sigma, gw, ga)    # (both from one pass)
        return (gs if ctx.needs_input_grad[0] else None), None, gl


class _SampleGeometryFunction(autograd.Function):
    @staticmethod
    def forward(ctx, origins, dirs, samples):
        ctx.samples = samples
        ctx.set_materialize_grads(False)                         # (a None upstream gradient stays None: the kernel's null pointer)
        ctx.save_for_backward(dirs)
        return samples.depth.clone(), samples.length.clone()     # (copies: autograd wants outputs of its own; no kernel of ours)

    @staticmethod
    def backward(ctx, grad_depth, grad_length):
        if not (ctx.needs_input_grad[0] or ctx.needs_input_grad[1]):
            return None, None, None
        (dirs,) = ctx.saved_tensors
        s = ctx.samples
        gd = None if grad_depth is None else grad_depth.contiguous()
        gl = None if grad_length is None else grad_length.contiguous()
        go, gdir = _X.sample_geometry_backward(s.offsets, s.face, s.depth, s.length, dirs.detach().contiguous(), gd, gl)
        return (go if ctx.needs_input_grad[0] else None), (gdir if ctx.needs_input_grad[1] else None), None


class _AccumulateFunction(autograd.Function):
    @staticmethod
    def forward(ctx, w, values, samples):
        w = w.contiguous()
        values = None if values is None else values.contiguous()
        out = _C.sample_accumulate(samples.offsets, w, values)
        ctx.samples = samples
        ctx.has_values = values is not None
        ctx.save_for_backward(*((w,) if values is None else (w, values)))
        return out

    @staticmethod
    def backward(ctx, grad_out):
        w = ctx.saved_tensors[0]
        values = ctx.saved_tensors[1] if ctx.has_values else None
        need_w, need_v = ctx.needs_input_grad[0], ctx.has_values and ctx.needs_input_grad[1]
        if not (need_w or need_v):
            return None, None, None
        s = ctx.samples
        gw, gv = _C.sample_accumulate_backward(s.ray, s.Q, w, values, grad_out.contiguous(), need_w, need_v)
        return gw, gv, None


def sample_geometry(samples: RaySamples, rays: Rays):
    """(depth, length), float32 [T]: the two list arrays of `samples`, same bits, as tensors that are differentiable in
    rays.origins and rays.dirs -- the geometric half of a gradient in the rays.  The forward launches no
    kernel.  `samples` must carry `face` (ray_samples(faces=True), or a select of such lists); `rays` are the Rays the
    samples were marched from, with explicit origins and dirs, float32 [Q, 3] on the samples' device.  Camera-mode and NDC
    rays are refused as points refuses them: pinhole_rays is torch and differentiable in c2w already.

    Both ends of a crossing lie on axis-aligned planes, z = (P_a - o_a) / d_a in the parameter along `dirs` as given, so
    dz/do_a = -1 / d_a and dz/dd_a = -z / d_a.  Backward, a lane per ray over its segment in list order, float32, no
    contraction, six accumulators from 0 (include/svoxt.h, svoxt_sample_geometry_bwd, is the definition), per sample with
    gz_in = g_depth - g_length and gz_out = g_length:

        a = entry;  if a < 3 and d[a] != 0:  u = gz_in  / d[a];  go[a] -= u;  gd[a] -= u * depth
        b = exit;   if          d[b] != 0:   v = gz_out / d[b];  go[b] -= v;  gd[b] -= v * (depth + length)

    Every ray's gradient is written (zeros without samples); no atomics, the same bits in every run.  It is the gradient
    of the two PLANES: two terms of the order of step_size are left out by definition -- depth of a later crossing is its
    plane's z plus one step_size * delta_scale, length holds another, and delta_scale depends on dirs.  The crossing set
    itself is piecewise constant in the rays.  The view-dependent half is view_basis in viewdirs and shade_samples in
    basis: with both, a rendered colour is differentiable in a camera pose."""
    if not isinstance(samples, RaySamples):
        raise RuntimeError("sample_geometry: samples must be a RaySamples")
    if samples.face is None:
        raise RuntimeError("sample_geometry: the samples carry no `face`: march them with ray_samples(faces=True) (select keeps "
                           "face; the lists of split and merge_samples have none: their pieces' ends are not leaf faces -- "
                           "carry depth[index] and length[index] over in torch instead)")
    if not isinstance(rays, Rays):
        raise RuntimeError("sample_geometry: rays must be the Rays the samples were marched from (camera-mode and NDC rays are "
                           "not served: pinhole_rays is differentiable in c2w already)")
    o, d = rays.origins, rays.dirs
    for name, x in (("origins", o), ("dirs", d)):
        if not isinstance(x, torch.Tensor) or x.dtype != torch.float32 or tuple(x.shape) != (samples.Q, 3):
            raise RuntimeError(f"sample_geometry: rays.{name} must be float32 [Q, 3] with Q = {samples.Q}, the rays the samples were marched from")
        if x.device != samples.ray.device:
            raise RuntimeError("sample_geometry: the rays must be on the device of the samples")
    _require_gpu("sample_geometry", samples, o, d)
    return _SampleGeometryFunction.apply(o, d, samples)


def sample_weights(samples: RaySamples, sigma, length=None):
    """(w float32 [T], alpha float32 [Q]) from a density per sample, differentiable in `sigma`:

        per ray, in list order:  att = exp(-(length * sigma));  w = T * (1 - att);  T *= att;      alpha = 1 - T_end

    A sample with sigma <= 0 gets w = 0, leaves T unchanged and receives no gradient, as the march skips it.  No
    thresholds and no early stop (the convention of the package's backwards).  With sigma = features[samples.row, -1]
    alpha has the bits of opacity_render and of render_depth_moments' third column.

    :param length: float32 [T] used in place of samples.length by the same operation sequence (length = samples.length:
        today's bits) -- sample_geometry's --, which makes the operator differentiable in it: grad_length[k] =
        sigma[k] * the bracket grad_sigma[k] multiplies by length[k], 0 where sigma <= 0; both from one pass."""
    if not isinstance(sigma, torch.Tensor) or sigma.dtype != torch.float32 or sigma.dim() != 1 or \
            not isinstance(samples, RaySamples) or sigma.shape[0] != len(samples):
        raise RuntimeError("sigma must be float32 [T], one entry per sample")
    if length is None:
        _require_gpu("sample_weights", samples, sigma)
        return _SampleWeightsFunction.apply(sigma, samples)
    if not isinstance(length, torch.Tensor) or length.dtype != torch.float32 or tuple(length.shape) != (len(samples),):
        raise RuntimeError("length must be float32 [T], one entry per sample")
    _require_gpu("sample_weights", samples, sigma, length)
    return _SampleWeightsFunction.apply(sigma, samples, length)


def accumulate(samples: RaySamples, w, values=None):
    """out float32 [Q, C]: out[q, c] = sum_k w[k] * values[k, c] over ray q's samples, added in list order; [Q], the plain
    sum of w, without `values`.  Differentiable in `w` and `values`."""
    if not isinstance(w, torch.Tensor) or w.dtype != torch.float32 or w.dim() != 1 or not isinstance(samples, RaySamples) \
            or w.shape[0] != len(samples):
        raise RuntimeError("w must be float32 [T], one entry per sample")
    if values is not None and (not isinstance(values, torch.Tensor) or values.dtype != torch.float32 or values.dim() != 2
                               or values.shape[0] != len(samples) or values.shape[1] < 1):
        raise RuntimeError("values must be float32 [T, C], one row per sample, C >= 1")
    _require_gpu("accumulate", samples, w, values)
    return _AccumulateFunction.apply(w, values, samples)


def composite(samples: RaySamples, sigma, values=None):
    """(out, alpha, w): accumulate(samples, w, values) with (w, alpha) = sample_weights(samples, sigma)."""
    w, alpha = sample_weights(samples, sigma)
    return accumulate(samples, w, values), alpha, w


# --------------------------------------------------------------------------------------- running values along a ray
class _RayScanFunction(autograd.Function):
    @staticmethod
    def forward(ctx, values, samples, op, exclusive, reverse):
        values = values.contiguous()
        ctx.samples, ctx.op, ctx.exclusive, ctx.reverse = samples, op, exclusive, reverse
        ctx.save_for_backward(values)
        return _X.ray_scan(samples.offsets, values, op, exclusive, reverse)

    @staticmethod
    @autograd.function.once_differentiable
    def backward(ctx, grad_out):
        if not ctx.needs_input_grad[0]:
            return None, None, None, None, None
        (values,) = ctx.saved_tensors
        grad = _X.ray_scan_backward(ctx.samples.offsets, values, ctx.op, ctx.exclusive, ctx.reverse, grad_out.contiguous())
        return grad, None, None, None, None


def ray_scan(samples: RaySamples, values, op: str = "sum", *, exclusive: bool = False, reverse: bool = False):
    """Running values along every ray, shaped like `values` (float32 [T] or [T, C]): per ray and channel, in list order
    (reverse: from the ray's last sample to its first), float32, no contraction:

        acc = 0 | 1 | -inf | +inf;   new = acc + v | acc * v | (v > acc) ? v : acc | (v < acc) ? v : acc     ("sum" | "prod" | "max" | "min")
        out = new   (exclusive: acc from before the step);   acc = new

    max / min never take a NaN and keep the first of equal values.  ray_scan(s, att, "prod", exclusive=True) is the
    transmittance in front of every sample; the last inclusive "sum" of a ray is accumulate(s, w), bit for bit.
    Differentiable in `values`, once: "sum" by the scan of the gradient in the other direction, "prod" by two sweeps
    without a division (zeros among the values are safe), "max" / "min" by sending every position's gradient to the
    sample that supplied its value -- fixed float32 sequences (include/svoxt.h), one entry per sample, no atomics."""
    if not isinstance(samples, RaySamples):
        raise RuntimeError("ray_scan: samples must be a RaySamples")
    if not isinstance(values, torch.Tensor) or values.dtype != torch.float32 or values.dim() not in (1, 2) \
            or values.shape[0] != len(samples) or (values.dim() == 2 and values.shape[1] < 1):
        raise RuntimeError("ray_scan: values must be float32 [T] or [T, C], one row per sample, C >= 1")
    if op not in _X.SCAN_OPS:
        raise RuntimeError(f"ray_scan: op must be one of {sorted(_X.SCAN_OPS)}")
    _require_gpu("ray_scan", samples, values)
    flat = values.dim() == 1
    out = _RayScanFunction.apply(values[:, None] if flat else values, samples, op, bool(exclusive), bool(reverse))
    return out[:, 0] if flat else out


def _quantiles(q, dev):
    """`q` (a number, a sequence or a tensor) -> float32 [nq] on `dev`, every value in [0, 1]."""
    if isinstance(q, torch.Tensor):
        if q.dtype != torch.float32:
            raise RuntimeError("ray_quantile: q must be a sequence or a float32 tensor of values in [0, 1]")
        t = q.detach()
    else:
        try:
            t = torch.tensor(q, dtype=torch.float32)
        except (TypeError, ValueError, RuntimeError):
            raise RuntimeError("ray_quantile: q must be a sequence or a float32 tensor of values in [0, 1]") from None
    if t.dim() == 0:
        t = t.reshape(1)
    if t.dim() != 1 or t.numel() < 1 or not bool(((t >= 0) & (t <= 1)).all()):
        raise RuntimeError("ray_quantile: q must hold nq >= 1 values in [0, 1]")
    return t.to(dev).contiguous()


def ray_quantile(samples: RaySamples, w, q, *, normalize: bool = True):
    """(index int64 [Q, nq], frac float32 [Q, nq]): where along every ray the running sum of `w` (float32 [T]) crosses
    each target.  Per ray, in list order, float32: a sample with w > 0 adds c = c + w from 0, any other (zero, negative,
    NaN) is passed over; target = q * c_end (normalize=False: q itself -- compositing weights, the mass 1 - alpha lying
    behind the volume); index is the list index in [0, T) of the first sample with w > 0 and c >= target, frac =
    (target - c_before) / w clamped to [0, 1], the position inside the crossing.  index = -1 and frac = 0 where the ray
    has no positive weight or the target is never reached.  `q`: a sequence or float32 tensor of nq >= 1 values in [0, 1].
    Not differentiable."""
    if not isinstance(samples, RaySamples):
        raise RuntimeError("ray_quantile: samples must be a RaySamples")
    if not isinstance(w, torch.Tensor) or w.dtype != torch.float32 or w.dim() != 1 or w.shape[0] != len(samples):
        raise RuntimeError("ray_quantile: w must be float32 [T], one entry per sample")
    qs = _quantiles(q, w.device)
    _require_gpu("ray_quantile", samples, w)
    with torch.no_grad():
        return _X.ray_quantile(samples.offsets, w.detach().contiguous(), qs, bool(normalize))


def quantile_depth(samples: RaySamples, w, q, *, normalize: bool = True, empty: float = float("nan")):
    """depth float32 [Q, nq] at the quantiles of ray_quantile: depth[index] + frac * length[index], `empty` where
    index < 0.  q = 0.5: the median depth."""
    index, frac = ray_quantile(samples, w, q, normalize=normalize)
    if len(samples) == 0:
        return torch.full_like(frac, float(empty))
    at = index.clamp(min=0)
    z = samples.depth[at] + frac * samples.length[at]
    return torch.where(index < 0, torch.full_like(z, float(empty)), z)


# ----------------------------------------------------------------------------------------- samples to rows and back
def _columns(dim, K, dev, what):
    """`dim` (None, int, slice, list or tensor, N3Tree.tv's convention) -> int32 distinct columns on `dev`, None for all."""
    if dim is None:
        return None
    if isinstance(dim, torch.Tensor):
        dim = dim.cpu()
    try:
        picked = torch.arange(K)[dim].reshape(-1)
    except (IndexError, TypeError) as e:
        raise RuntimeError(f"{what}: dim does not select columns of a table of {K}: {e}") from None
    if picked.numel() == 0:
        raise RuntimeError(f"{what}: dim selects no column")
    if picked.unique().numel() != picked.numel():
        raise RuntimeError(f"{what}: dim selects a column twice")
    return picked.to(device=dev, dtype=torch.int32)


class _GatherRowsFunction(autograd.Function):
    @staticmethod
    def forward(ctx, table, samples, cols):
        ctx.samples, ctx.cols, ctx.shape = samples, cols, tuple(table.shape)
        return _C.sample_gather_rows(table.contiguous(), samples.row, cols)

    @staticmethod
    def backward(ctx, grad_out):
        if not ctx.needs_input_grad[0]:
            return None, None, None
        M, K = ctx.shape
        plan = ctx.samples.row_plan(M)
        return _C.sample_reduce_rows(grad_out.contiguous(), plan.arrays, "sum", 0.0, ctx.cols, K), None, None


class _ReduceRowsFunction(autograd.Function):
    @staticmethod
    def forward(ctx, values, samples, M, op, empty):
        plan = samples.row_plan(M)
        ctx.samples, ctx.plan, ctx.op = samples, plan, op
        return _C.sample_reduce_rows(values.contiguous(), plan.arrays, op, empty)

    @staticmethod
    def backward(ctx, grad_out):
        if not ctx.needs_input_grad[0]:
            return None, None, None, None, None
        g = grad_out
        if ctx.op == "mean":                                    # (rows without a sample are gathered by no one)
            g = g / ctx.plan.counts.clamp(min=1).to(torch.float32)[:, None]
        return _C.sample_gather_rows(g.contiguous(), ctx.samples.row, None), None, None, None, None


def gather_rows(samples: RaySamples, table, dim=None):
    """out float32 [T, C]: out[k, j] = table[samples.row[k], cols[j]] -- the feature row of every sample.  `dim` selects
    the columns as N3Tree.tv's does (int, slice, list or tensor of distinct columns; None: all K); the column axis is
    kept, gather_rows(s, features, dim=-1)[:, 0] is sigma.  A sample whose row is outside [0, M) gets zeros.

    Differentiable in `table`: the gradient is a full [M, K] table, reduce_rows(op="sum") of the upstream gradient at
    the selected columns and 0 everywhere else, summed per row in the fixed order of include/svoxt.h over the cached
    row plan -- no atomics, the same bits in every run."""
    _require_gpu("gather_rows", samples, table if isinstance(table, torch.Tensor) else None)
    if not isinstance(table, torch.Tensor) or table.dtype != torch.float32 or table.dim() != 2 or table.shape[1] < 1:
        raise RuntimeError("gather_rows: table must be float32 [M, K], K >= 1")
    cols = _columns(dim, table.shape[1], table.device, "gather_rows")
    return _GatherRowsFunction.apply(table, samples, cols)


def reduce_rows(samples: RaySamples, values, M: int, op: str = "sum", empty: float = 0.0):
    """out float32 [M, C] from per-sample values float32 [T, C] ([T]: the result is [M]): per feature row the "sum",
    "mean", "max" or "min" over the samples that name it, `empty` for rows without a sample.  Gather only, in the order
    include/svoxt.h defines: samples in ascending index; a sum in chunks of 256 samples, each added sequentially from
    0, the chunks' partials added in chunk order (the plain sequential sum up to 256 samples); the mean divides that
    sum once by the count; max / min are NaN as soon as one value of the row is.  Samples whose row is outside [0, M)
    take no part.  "sum" and "mean" are differentiable in `values` (the gradient is gather_rows of the upstream
    gradient, divided by the row's count for the mean); "max" and "min" return a tensor without gradient."""
    _require_gpu("reduce_rows", samples, values if isinstance(values, torch.Tensor) else None)
    if not isinstance(values, torch.Tensor) or values.dtype != torch.float32 or values.dim() not in (1, 2) \
            or values.shape[0] != len(samples) or (values.dim() == 2 and values.shape[1] < 1):
        raise RuntimeError("reduce_rows: values must be float32 [T] or [T, C], one row per sample, C >= 1")
    if op not in _C._extras.ROWS_OPS:
        raise RuntimeError(f"reduce_rows: op must be one of {sorted(_C._extras.ROWS_OPS)}")
    M = _C._extras._check_rows_extent(M, "reduce_rows")
    empty = float(empty)
    flat = values.dim() == 1
    v = values[:, None] if flat else values
    if op in ("max", "min"):
        out = _C.sample_reduce_rows(v.detach().contiguous(), samples.row_plan(M).arrays, op, empty)
    else:
        out = _ReduceRowsFunction.apply(v, samples, M, op, empty)
    return out[:, 0] if flat else out
