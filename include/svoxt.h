/* svoxt.h -- C ABI of libsvoxt_hip.so, the MI355X (gfx950) implementation of
 * svox_t's differentiable volume-render hot path.
 *
 * This is the drop-in boundary: plain pointers and sizes, no torch / pybind
 * types.  Each entry point replaces one function of the reference's pybind11
 * module `svox_t.csrc` (reference paths are relative to the svox_t checkout):
 *
 *   svoxt_volume_render_fwd   <- volume_render            svox_t/csrc/svox.cpp:55,128   (rt_kernel.cu:1362-1379)
 *   svoxt_volume_render_bwd   <- volume_render_backward   svox_t/csrc/svox.cpp:57,130   (rt_kernel.cu:1402-1426)
 *   svoxt_opacity_render_fwd  <- opacity_render           svox_t/csrc/svox.cpp:68,138   (rt_kernel.cu:1574-1591)
 *   svoxt_opacity_render_bwd  <- opacity_render_backward  svox_t/csrc/svox.cpp:69,139   (rt_kernel.cu:1593-1616)
 *   svoxt_render_depth        <- render_depth             svox_t/csrc/svox.cpp:63,134   (rt_kernel.cu:1506-1523)
 *   svoxt_query_fwd           <- query_vertical           svox_t/csrc/svox.cpp:45,119   (svox_kernel.cu:274-324)
 *   svoxt_query_bwd           <- query_vertical_backward  svox_t/csrc/svox.cpp:46,120   (svox_kernel.cu:380-402)
 *   svoxt_p2v_fwd             <- p2v                      svox_t/csrc/svox.cpp:52,125   (p2v_kernel.cu:240-261)
 *   svoxt_p2v_bwd             <- p2v_backward             svox_t/csrc/svox.cpp:53,126   (p2v_kernel.cu:263-285)
 *   svoxt_quantize_median_cut <- quantize_median_cut      svox_t/csrc/svox.cpp:71,144   (quantizer.cpp:130-157)
 *   svoxt_tree / svoxt_rays / svoxt_options
 *                             <- TreeSpec / RaysSpec / RenderOptions
 *                                                         svox_t/csrc/include/data_spec.hpp:52-145
 *
 * Entry points without a counterpart in the reference, all optional and
 * result-neutral (a caller that ignores them gets the same numbers, slower):
 *   svoxt_accel_build / svoxt_accel_bytes            cached prefix of the root descent
 *   svoxt_ray_order                                  coherent order for ray batches that are not images
 *   svoxt_volume_render_fwd_record / _bwd_replay     backward without tree traversal
 *   svoxt_can_record, svoxt_bwd_workspace_bytes, svoxt_compact_rows(_clear), svoxt_count_fwd,
 *   svoxt_query_leaves (the reference's mask compaction, made deterministic)
 *
 * Conventions
 *   - Every pointer marked "device" is HBM memory of the current HIP device;
 *     the caller owns all buffers (inputs are borrowed, outputs are written in
 *     place, nothing is allocated or freed by the library).
 *   - `stream` is a hipStream_t passed as void* (NULL = the null stream).  All
 *     calls are asynchronous with respect to the host: they enqueue work and
 *     return; no call synchronises.
 *   - Return value 0 = success; otherwise one of SVOXT_ERR_* and
 *     svoxt_last_error() describes the failure (thread-local string).
 *     Unlike the reference (which only printf's launch errors,
 *     svox_t/csrc/include/common.cuh:108-111) launch failures are returned.
 *   - fp32 only (the reference dispatches fp64 nominally, but every Python
 *     path builds fp32 tensors).
 */
#ifndef SVOXT_H_
#define SVOXT_H_

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SVOXT_ABI_VERSION 22

enum {
    SVOXT_OK = 0,
    SVOXT_ERR_INVALID = 1,      /* null pointer, bad extent, inconsistent options */
    SVOXT_ERR_UNSUPPORTED = 2,  /* valid for the reference, not implemented here  */
    SVOXT_ERR_HIP = 3           /* HIP runtime / launch failure                   */
};

/* Alignment.  A device pointer is aligned to its element (4 bytes for float / int32, 8 for int64) unless its entry
 * point asks for more; a tensor may start anywhere in a larger buffer (flat[1:], a slice of a checkpoint blob).
 * No entry point issues a 16-byte access through a caller's pointer that is not 16-byte aligned:
 *   - The entry points whose kernels read tree.features as 16-byte vectors when K % 4 == 0 -- the colour render
 *     (svoxt_volume_render_fwd / _fwd_ws / _fwd_scratch / _fwd_record, svoxt_volume_render_bwd / _bwd_replay), the
 *     svoxt_step_* calls of a payload that is not padded, and svoxt_exp_table_build -- REFUSE such a table (and a
 *     tree.exp_table) that is not 16-byte aligned: SVOXT_ERR_INVALID before any launch, svoxt_last_error() names the
 *     function and the 16-byte requirement.  K % 4 != 0: rows are read float by float, any 4-byte alignment will do.
 *     This was undefined before and is an error now: the ABI version is unchanged.
 *   - The operators that read sigma alone take 4-byte alignment for every K: opacity (forward, backward, replay), depth,
 *     depth moments, distortion, svoxt_ray_samples_*, the row-plan backward (svoxt_render_grad_rows_*), query, count, the
 *     sigma bitmask, and the motion operators (their joint-feature rows are 16-byte reads of the aligned workspace).
 *   - The operators that move or write whole rows choose a 16-byte or a 4-byte route from the pointers they get and give
 *     the same bits either way, writing nothing outside the table: svoxt_assign_leaves, svoxt_prune_gather_rows,
 *     svoxt_gather_rows, svoxt_shade_samples_fwd, svoxt_frontier_reduce, svoxt_compact_rows, svoxt_optim_step,
 *     svoxt_interp_stencil (its outputs), svoxt_interp_rows_fwd, svoxt_interp_points_bwd.
 *     svoxt_frontier_diam chooses likewise (from features AND data), but its two routes add a pair's squared differences
 *     in different orders: results agree within float32 rounding of the sum, not bit for bit (the Python layer hands it
 *     aligned copies of both, so that one table gives one result wherever it starts).
 *   - Workspaces, sample lists and matrix_out of svoxt_warp_vertices state their own alignment where they are declared.
 * The Python operator layer (svox_t_amd.csrc) accepts any contiguous tensor: its colour render hands over an aligned copy
 * of a feature table with K % 4 == 0 that starts off a 16-byte boundary (one integer test per call for an aligned one). */

/* enum DataFormat, svox_t/csrc/include/data_spec.hpp:45-50 */
enum {
    SVOXT_FORMAT_RGBA = 0,
    SVOXT_FORMAT_SH = 1,
    SVOXT_FORMAT_SG = 2,
    SVOXT_FORMAT_ASG = 3
};

/* TreeSpec (data_spec.hpp:67-111) as the kernels need it.  `data` is NOT the
 * feature storage: it holds, per leaf slot, the row index into `features`; a
 * slot is empty iff its index >= M (rt_kernel.cu:269). */
typedef struct svoxt_tree {
    const float*   features;     /* device [M, K] row-major; row = colour/SH coeffs..., sigma last; 16-byte aligned where
                                    K % 4 == 0 and the entry point reads whole rows ("Alignment" above) */
    int64_t        M;
    int32_t        K;            /* data_dim */
    int32_t        N;            /* branching factor per axis (2 = octree) */
    const int32_t* data;         /* device [capacity, N, N, N, 1] feature-row index per slot */
    const int32_t* child;        /* device [capacity, N, N, N] relative child offset, 0 = leaf */
    int64_t        n_internal;   /* rows of child/data in use (TreeSpec.n_internal) */
    const float*   offset;       /* device [3]  world -> tree: p' = offset + scaling * p */
    const float*   scaling;      /* device [3] */
    const float*   extra_data;   /* device [extra_rows, extra_cols] SG/ASG lobes, or NULL */
    int32_t        extra_rows;
    int32_t        extra_cols;
    float*         weight_accum; /* device [capacity * N^3] or NULL (TreeSpec._weight_accum) */
    const float*   xform;        /* device [M,d,d] TreeSpec.transformation_matrices (per-leaf rotation of the view
                                    direction by the upper-left 3x3, rt_kernel.cu:283-291) or NULL;
                                    volume_render fwd/bwd only (ignored by the other entry points); d = xform_dim below */
    const void*    accel;        /* device, optional: acceleration grid built by svoxt_accel_build for THIS
                                    child/data content (N == 2), or NULL.  Pure cache: results are identical
                                    with or without it; rebuild after any change to child or data. */
    int32_t        accel_log2;   /* log2 of the grid resolution per axis the grid was built with, | SVOXT_ACCEL_BRICKS
                                    if it was built in that layout (the value handed to svoxt_accel_build) */
    int32_t        xform_dim;    /* rows = columns of each xform matrix: 3, or 4 (the [M,4,4] that
                                    warp_vertices / blend_transformation_matrix produce); 0 means 3 */
    const void*    sigma_mask;   /* device, optional: one bit per feature row, set iff the row's sigma (its last
                                    float) > sigma_mask_thresh, built by svoxt_sigma_mask_build for THIS feature
                                    content, or NULL.  Pure cache like accel (results are identical with or
                                    without it; rebuild after any change to the features): the two-kernel
                                    forward's march reads a bit instead of gathering sigma. Ignored unless
                                    sigma_mask_thresh == options.sigma_thresh. */
    float          sigma_mask_thresh;
    int32_t        reserved0;    /* 0 */
    const float*   exp_table;    /* device, optional (ABI v17; RGBA-style rows of K = 8 / 16 / 32 floats only): [M, K], entry (row, c)
                                    = the exponential exp(-features[row][c]) exactly as the kernels form it, for the K - 1
                                    feature columns, and sigma itself in the last column, built by svoxt_exp_table_build for
                                    THIS feature content, or NULL.  Pure cache like accel and sigma_mask (results are
                                    identical with or without it): the sigmoids of such a payload do not depend on the view,
                                    so the shade kernel of the two-kernel forward and both sweeps of the per-tile backward
                                    read the table instead of forming the exponential once per sample. */
} svoxt_tree;

/* RaysSpec (data_spec.hpp:52-65); with c2w set, CameraSpec (data_spec.hpp:113-126):
 * the image-mode entry points volume_render_image / volume_render_image_backward
 * (rt_kernel.cu:1382-1399, 1428-1452) are every render call below given a camera. */
typedef struct svoxt_rays {
    const float* origins;        /* device [Q, 3] */
    const float* dirs;           /* device [Q, 3] */
    const float* vdirs;          /* device [Q, 3] */
    int64_t      Q;
    int32_t      image_width;    /* optional hint (no counterpart in the reference): if the batch is a   */
    int32_t      image_height;   /* row-major W x H image (Q == W*H, both multiples of 8) the kernels walk
                                    it in 8x8 pixel tiles -- row-major, or in super-tiles of 8 x 8 tiles where the
                                    tree has more than 2^21 feature rows (a rule of M alone: a forward that
                                    records sample lists and the backward that walks them use the same walk);
                                    0 = no hint.  Results do not depend on it. */
    const float* c2w;            /* camera mode when non-NULL: device camera-to-world matrix, rows of 4 floats
                                    ([3,4] or [4,4] contiguous).  Ray q is then pixel (q % image_width,
                                    q / image_width) of a pinhole camera, generated inside the kernels as
                                    cam2world_ray + maybe_world2ndc do (rt_kernel.cu:1153-1190; the NDC warp
                                    applies iff options.ndc_width >= 0, and the view direction is the one
                                    before the warp, :1203); origins / dirs / vdirs are ignored, Q must be
                                    image_width * image_height, outputs are the [H, W, C+1] image. */
    float        fx, fy;         /* focal lengths in pixels (camera mode) */
    const int32_t* order;        /* optional (ABI v15, no counterpart in the reference): device int32 [Q], a permutation
                                    of 0 .. Q-1 (svoxt_ray_order's): launch thread i works on ray order[i], so
                                    that the 64 rays of a wavefront are the ones the permutation puts next to
                                    each other -- nothing is gathered or scattered, every ray's inputs and results
                                    stay at the ray's own index.  Sample lists recorded with an order must be
                                    replayed with the same one.  NULL: thread i takes ray i (or the image tiles
                                    above); not allowed together with the image hint or camera mode. */
} svoxt_rays;

/* RenderOptions (data_spec.hpp:129-145), same fields in the same order. */
typedef struct svoxt_options {
    float   step_size;
    float   background_brightness;
    int32_t format;
    int32_t basis_dim;
    int32_t ndc_width;
    int32_t ndc_height;
    float   ndc_focal;
    int32_t min_comp;
    int32_t max_comp;
    float   sigma_thresh;
    float   stop_thresh;
} svoxt_options;

int         svoxt_abi_version(void);
const char* svoxt_last_error(void);

/* get_out_data_dim (rt_kernel.cu:1352-1358): number of output columns C+1 of
 * volume_render for a feature width K. Returns -1 for invalid options. */
int svoxt_out_data_dim(const svoxt_options* opt, int32_t K);

/* out: device [Q, C+1], fully written (no pre-zeroing needed). */
int svoxt_volume_render_fwd(const svoxt_tree* tree, const svoxt_rays* rays,
                            const svoxt_options* opt, float* out, void* stream);

/* The same result (bit for bit) with device scratch: with svoxt_fwd_workspace_bytes(Q, S)
 * bytes (S >= 8, 96 is a good value) the forward can run as two kernels -- one that only
 * steps the rays through the tree and lists each ray's samples (up to S; longer rays finish in a
 * tail launch), one that shades the lists: per 64-ray tile with eight wavefronts sharing the
 * work (3-channel payloads; only on request: svoxt_volume_render_fwd_scratch with SVOXT_LISTS_FWD_TWO_KERNELS), or with the channels of a row on
 * the lanes of a wavefront (RGBA-style rows of 8 / 16 / 32 floats: the default for them) --
 * instead of one kernel as long as its longest ray (NOTEBOOK.md 5).  Other payloads,
 * tree->weight_accum, a NULL or too small workspace: exactly svoxt_volume_render_fwd.  Contents of the workspace on return are unspecified.
 * (Reference: volume_render, rt_kernel.cu:1362-1379; trace_ray :222-328.) */
/* flags: 0, or an OR of the SVOXT_LISTS_* values below (how the scratch lists are filled); among them
 * SVOXT_FWD_FAST_SIGMOID (= SVOXT_LISTS_NATIVE_MATH) -- an opt-in tolerance mode for
 * RGBA-style rows of 8 / 16 / 32 floats: bit-exact stepping, but expf and the per-channel quotient
 * w / (1 + exp(-x)) -- double precision in the reference (rt_kernel.cu:280, 300-305) -- are taken with the
 * hardware's v_exp_f32 / v_rcp_f32.  Outputs within 1e-5 relative (tests at full size); no longer bit for bit. */
#define SVOXT_FWD_FAST_SIGMOID 1
int64_t svoxt_fwd_workspace_bytes(int64_t Q, int32_t max_samples);
int svoxt_volume_render_fwd_ws(const svoxt_tree* tree, const svoxt_rays* rays,
                               const svoxt_options* opt, float* out,
                               void* workspace, int64_t workspace_bytes, int32_t flags, void* stream);
/* The same with the scratch given as a svoxt_sample_lists (declared below; rec / aux, optionally
 * pooled through blocktab): what svoxt_volume_render_fwd_ws does with a dense workspace, for callers
 * that want the pool.  The lists come back in an unspecified state: they serve no backward (early
 * termination applies while they are written). */
struct svoxt_sample_lists;
int svoxt_volume_render_fwd_scratch(const svoxt_tree* tree, const svoxt_rays* rays,
                                    const svoxt_options* opt, float* out,
                                    const struct svoxt_sample_lists* scratch, int32_t flags, void* stream);

/* grad_out: device [Q, grad_cols] with grad_cols = C+1.
 * grad_features: device [M, grad_stride] floats of which columns 0..K-1 are the
 *           gradient; zeroed by this call on `stream`, then accumulated with
 *           float atomics (as the reference: zeros_like + atomicAdd,
 *           rt_kernel.cu:1415,413,486).  grad_stride = 0 or K is the
 *           reference's dense [M, K]; a stride that makes rows start on 64-byte
 *           boundaries (e.g. 32 for K = 28: rows of 128 bytes) lets each row's
 *           atomics hit two memory-side requests (the rate those are taken at is
 *           what bounds the backward): 2 instead of 2.75 on average for the
 *           one-kernel backward, 2 instead of 3.7 for the two-kernel one (its second
 *           kernel 0.30 -> 0.20 ms); svoxt_compact_rows turns the result into the
 *           dense table (0.03 ms for 75 MB).
 * workspace: device scratch of `workspace_bytes` bytes, or NULL.  With
 *           svoxt_bwd_workspace_bytes(Q, S) bytes the first pass records up to
 *           S composited samples per ray (8 bytes each) and the second pass
 *           replays them instead of traversing the tree a second time; rays
 *           with more samples than S march the remainder, so any S >= 0 gives
 *           the same result.  Contents on return are unspecified. */
int64_t svoxt_bwd_workspace_bytes(int64_t Q, int32_t max_samples);
int svoxt_volume_render_bwd(const svoxt_tree* tree, const svoxt_rays* rays,
                            const svoxt_options* opt, const float* grad_out,
                            int32_t grad_cols, float* grad_features, int32_t grad_stride,
                            void* workspace, int64_t workspace_bytes, void* stream);

/* Sample lists (no counterpart in the reference).  When a forward will be
 * followed by a backward, the forward can record which samples each ray
 * composited -- 8-byte records (feature row, step length), the k-th record of the ray
 * handled by launch thread t at rec[block(t / 64, k / 8)][t % 64][k % 8] (a lane's 8
 * consecutive records are one 64-byte line; `block` is the identity for dense lists and
 * goes through blocktab for pooled ones, below), and aux[q] = (count, overflow flag,
 * resume point, final transmittance) -- and the backward then replays
 * those samples instead of traversing the tree again (twice, in the reference:
 * rt_kernel.cu:365-494).  Rays with more than max_samples composited samples
 * march the remainder, so the result does not depend on max_samples.  The lists hold EVERY
 * sample with sigma > 0 to the end of the ray -- what the reference's backward takes, which ignores
 * both thresholds (rt_kernel.cu:382, 456) -- and the recording forward applies its own rules while it
 * composites (ABI v20: sigma > sigma_thresh, :279; nothing after T <= stop_thresh, :313-319), so any
 * thresholds are served (`fast=True`); a sigma bitmask handed to a recording forward must be the one of
 * threshold 0.  Needs one of the specialised payloads (svoxt_can_record returns 1; with tree->xform
 * set: SH payloads on N = 2 trees); the lists are valid for the tree, features'
 * sign of sigma, rays and options they were recorded with.
 * svoxt_can_record returns 2 (r03) for SG / ASG payloads with 1 / 4 / 9 / 16 / 25 lobes and three channels on
 * N = 2 trees: their lists are recorded only TOGETHER WITH the exact per-tile backward's hand-over (lists.terms
 * given; svoxt_fwd_fills_terms says 3) and serve that backward alone (svoxt_volume_render_bwd_replay with
 * coef_bytes < 0, terms_state 3, fwd_out NULL); any other combination is SVOXT_ERR_UNSUPPORTED -- call the
 * marching svoxt_volume_render_bwd instead. */
/* svoxt_sample_lists.flags (ABI v16): how the kernels that write and read these lists work.
 *   SVOXT_LISTS_NATIVE_MATH      opt-in TOLERANCE mode for RGBA-style rows of 8 / 16 / 32 floats (= the `flags`
 *                                value SVOXT_FWD_FAST_SIGMOID of the scratch forwards): the stepping -- which
 *                                leaves a ray crosses, the step lengths, the lists -- stays bit-exact, the SHADING
 *                                arithmetic uses the hardware's exponential (v_exp_f32 on x * log2 e) and
 *                                reciprocal (v_rcp_f32) where the reference has expf and a double-precision
 *                                quotient (rt_kernel.cu:280, 300-305, 397, 408-425, 461-476): the channel-lane
 *                                shade / tail kernels of the forward and both sweeps of the per-tile backward.
 *                                Outputs within 1e-5 relative (+1e-6 absolute), gradients within 1e-5 of the
 *                                tight scale (tests at full size); not bit for bit.  A backward must be given the
 *                                flags its forward recorded with.  Ignored by every other payload / kernel.
 *   SVOXT_LISTS_FWD_ONE_KERNEL   the forward that fills these lists runs as one kernel / as march + shade
 *   SVOXT_LISTS_FWD_TWO_KERNELS  kernels where both exist (neither: the library's default for the payload:
 *                                two kernels for rows of 8 / 16 / 32 floats and for 3-channel forwards that
 *                                also fill `terms`).  Result-neutral. */
#define SVOXT_LISTS_NATIVE_MATH 1
#define SVOXT_LISTS_FWD_ONE_KERNEL 2
#define SVOXT_LISTS_FWD_TWO_KERNELS 4
/*   SVOXT_LISTS_FWD_NO_OVERLAP   march and shade of the two-kernel forward as two launches even where lists.tile_state
 *                                would let one launch carry both (below).  Result-neutral. */
#define SVOXT_LISTS_FWD_NO_OVERLAP 8
/*   SVOXT_LISTS_GRAD_ZEROED      (read by svoxt_volume_render_bwd_replay) grad_features is all zeros on entry and the call
 *                                need not fill it: the caller keeps a padded gradient scratch between steps and turns
 *                                it into the dense [M, K] gradient with svoxt_compact_rows_clear, which leaves it zeroed
 *                                again -- a fill of M * grad_stride floats per step less.  The caller answers for the
 *                                zeros (a scratch a failed call may have left half written must be filled again). */
#define SVOXT_LISTS_GRAD_ZEROED 16
/*   SVOXT_LISTS_BEGUN            (read by the recording forwards; ABI v18) blocktab, pool_next and tile_state hold -1
 *                                in every word already (svoxt_sigma_mask_build_fill on the same stream): the call
 *                                does not fill them again. */
#define SVOXT_LISTS_BEGUN 32
/*   SVOXT_LISTS_WALK_ROWMAJOR    (ABI v20) the order in which an image's 8 x 8 tiles are walked when these lists are written
 *   SVOXT_LISTS_WALK_SUPER       and read (svoxt_rays.image_width): lists are indexed by (tile, lane), so the backward that
 *                                replays them must walk the image the way the recording forward did.  Neither bit: the
 *                                library's rule (a function of tree->M and svoxt_set_super_tile_rows) at the time of EACH
 *                                call -- the caller answers for both calls seeing the same rule.  One bit set (what
 *                                svoxt_image_walk returns for the recording call: pass it to both): that walk, whatever
 *                                the rule says by the time of the backward. */
#define SVOXT_LISTS_WALK_ROWMAJOR 64
#define SVOXT_LISTS_WALK_SUPER 128
/* Test and measurement switches of the one-launch forward (fwd_roles_kernel; ABI v17), all result-neutral: its shading
 * workgroups drop every third tile they take / give up after one poll / treat what they load for every fifth tile as a
 * stale read would look -- the fallback launch must then deliver the same pixels, lists and hand-over -- and
 * SVOXT_LISTS_FWD_AGENT_FENCE: the march -> shade hand-over with an agent-scope release before the queue entry is
 * stored and an agent-scope acquire before the first load (the microarchitecture guide's valid form in full; the
 * default rests on same-XCD queues, acknowledged stores and sc1 loads, checked by a per-tile checksum). */
#define SVOXT_LISTS_TEST_DROP 256
#define SVOXT_LISTS_TEST_NOPOLL 512
#define SVOXT_LISTS_TEST_STALE 1024
#define SVOXT_LISTS_FWD_AGENT_FENCE 2048
typedef struct svoxt_sample_lists {
    void*   rec;           /* device, 64-byte aligned, max_samples * ceil(Q / 64) * 64 * 8 bytes: record k of the
                              ray handled by launch thread t lives at rec[t / 64][k / 8][t % 64][k % 8] (8 bytes
                              each): a lane's 8 consecutive records are one 64-byte line, written at once */
    void*   aux;           /* device, Q * 16 bytes: count | overflow, resume point, final transmittance, pad */
    int32_t max_samples;   /* S: a multiple of 8 in [8, 4096] */
    void*   coef;          /* device, coef_bytes >= max_samples * Q * 16 bytes (twice that with tree->xform:
                              the second half takes each sample's rotated view direction), 16-byte
                              aligned, or NULL.  Only read by
                              svoxt_volume_render_bwd_replay: with it (3-channel payloads of at most 32
                              floats per row, N = 2) the backward runs as two kernels -- the list walk
                              leaves each sample's contribution in factored form in rec / coef (rec is
                              overwritten), and a second kernel adds them up per 8x8 tile in LDS, so a
                              gradient row goes to memory once per tile instead of once per sample. */
    int64_t coef_bytes;    /* size of coef (a buffer too small for the route is ignored; a buffer that is given
                              selects the two-kernel form); -1 with coef NULL: take the per-tile route if it
                              can run as ONE kernel (no view rotations, fwd_out given: list walk and merge
                              fused, nothing goes through coef), else the one-kernel backward */
    void*   terms;         /* device, 16-byte aligned, terms_bytes >= 2 * the bytes of rec (16 per record slot), or NULL:
                              (att, e_0, e_1, e_2) of every 3-channel sample as the exact backward (fwd_out NULL,
                              the ONE-kernel form) needs them.  Given to svoxt_volume_render_fwd_record, the
                              one-kernel forward fills it (svoxt_fwd_fills_terms says whether it will); the
                              backward, told so by terms_state = 2 or 3 (what svoxt_fwd_fills_terms returned:
                              the layout the forward wrote), then gathers no feature row and forms no
                              exponential in either of its sweeps.  terms_state = 0 (3-channel payloads, since ABI v17): the
                              buffer is ignored and both sweeps gather the rows.  Same bits every way.
                              RGBA rows of 8 / 16 / 32 floats (C = 7 / 15 / 31): scratch between the two sweeps of
                              their exact backwards, 8 bytes per record slot for the per-tile kernel (attenuation,
                              second-pass total_color), 4 for the per-ray one; NULL or smaller: the per-ray list
                              replay that forms every sigmoid twice. */
    int64_t terms_bytes;
    /* Pooled lists (optional, ABI v12).  blocktab NULL: dense -- rec holds max_samples slots for every
     * ray, as described above.  blocktab given: device int32 [ceil(Q / 64) * max_samples / 8]; entry
     * (tile, b) names the 4 KB block of `rec` that holds records 8b .. 8b+7 of the tile's 64 rays
     * (-1: none).  The forward clears the table and hands blocks out of rec's pool_blocks blocks
     * (a positive multiple of 32: the pool is cut into 32 parts, a tile draws from part tile % 32;
     * pool_next: device int32 [32 * 16], one counter per part, 64 bytes apart, each = blocks handed out - 1
     * (word 1, ABI v18: 1 once a recording kernel has filled a ray's list to its capacity -- what the tail launches
     * read instead of every ray's list length; -1 after the fill);
     * placed right behind blocktab, table and counters are cleared with one fill) the first time a ray
     * of a tile starts block b; a ray that finds
     * the pool used up stops recording there exactly as one that reaches max_samples does (it marches
     * the rest).  rec then needs pool_blocks * 4096 bytes -- the samples that exist, not the cap times
     * the rays -- and max_samples (<= 512) only caps a single ray. */
    void*   blocktab;
    int64_t pool_blocks;
    void*   pool_next;
    int32_t terms_state;   /* see terms */
    int32_t flags;         /* 0 or an OR of SVOXT_LISTS_* (above) */
    void*   tile_state;    /* optional (pooled lists only): device int32 [17 * ceil(Q / 64) + 514], 8-byte aligned (its ready
                              queues hold 64-bit entries; a misaligned pointer is SVOXT_ERR_INVALID), scratch.  Given, the two-kernel
                              forward of 3-channel payloads (N = 2, no view rotations, sigma bitmask at hand) runs its march
                              and its shade as ONE launch: tiles are shaded in the order their marches finish, beside the
                              marches still running (per-tile states, then per-XCD ready queues of 64-bit entries -- tile id and a
                              checksum of the tile's lists -- and their counters: fwd_roles_kernel; NOTEBOOK.md step 33).  Cleared by the
                              forward together with the block table (one fill when it lies right behind pool_next's
                              counters).  Same lists, terms and pixels bit for bit.  NULL: two launches. */
} svoxt_sample_lists;

int svoxt_can_record(const svoxt_tree* tree, const svoxt_options* opt);
/* What svoxt_volume_render_fwd_record does with lists that carry `terms` for this tree / options / lists.flags:
 * 0 = nothing, 2 / 3 = fills them (in the layout of that number: pass it back as terms_state to the backward) */
int svoxt_fwd_fills_terms(const svoxt_tree* tree, const svoxt_options* opt, int32_t list_flags);

/* The sigma bitmask of svoxt_tree.sigma_mask (no counterpart in the reference): bytes for M rows, and the
 * build -- bit (row & 31) of 32-bit word (row >> 5) = features[row * K + K - 1] > sigma_thresh.  One read of a
 * 64-byte line per row (0.05 ms for 4.7 M rows of 32 floats); worth it where the feature table no longer fits
 * the Infinity Cache (see NOTEBOOK.md, step 26). */
int64_t svoxt_sigma_mask_bytes(int64_t M);
int svoxt_sigma_mask_build(const svoxt_tree* tree, float sigma_thresh, void* mask, void* stream);
/* ... and, in the same launch (ABI v18), fill_bytes bytes at `fill` (device, 16-byte aligned, a multiple of 16) set to
 * 0xff: the state a recording forward's pooled lists start from (blocktab, pool_next and tile_state, allocated in one
 * piece).  A caller that builds the mask right before a recording forward hands the lists over with
 * SVOXT_LISTS_BEGUN and saves that forward's own fill launch. */
int svoxt_sigma_mask_build_fill(const svoxt_tree* tree, float sigma_thresh, void* mask, void* fill, int64_t fill_bytes,
                                void* stream);
/* The exponentials table of svoxt_tree.exp_table (ABI v17; no counterpart in the reference) for RGBA-style rows of
 * 8 / 16 / 32 floats: table <- device float [M, K], 16-byte aligned, and -- in the same pass over the feature table --
 * the sigma bitmask (mask as for svoxt_sigma_mask_build, or NULL).  Rebuild after any change to the features. */
int svoxt_exp_table_build(const svoxt_tree* tree, float sigma_thresh, void* mask, float* table, void* stream);
int svoxt_volume_render_fwd_record(const svoxt_tree* tree, const svoxt_rays* rays,
                                   const svoxt_options* opt, float* out,
                                   const svoxt_sample_lists* lists, void* stream);
int svoxt_volume_render_bwd_replay(const svoxt_tree* tree, const svoxt_rays* rays,
                                   const svoxt_options* opt, const float* grad_out,
                                   int32_t grad_cols, float* grad_features, int32_t grad_stride,
                                   const svoxt_sample_lists* lists, const float* fwd_out, void* stream);
/* fwd_out: device [Q, C+1] = the output svoxt_volume_render_fwd_record produced
 * with these lists, or NULL.  NULL: two list walks per ray, every gradient
 * contribution bit-identical to the reference's formulas.  Given: ONE walk --
 * the reference's first pass only computes accum = sum_c g_c * out_c and the
 * final transmittance, both known from the forward; the value of accum then
 * differs from the sequentially accumulated one by float rounding (~1e-7 of the
 * summed magnitudes), which reaches the sigma column only (well inside the 1e-5
 * parity tolerance); colour gradients stay bit-identical. */

/* Copy the first K columns of src [M, stride] into dense dst [M, K] (streaming,
 * non-temporal): turns a strided gradient buffer into the reference's layout. */
int svoxt_compact_rows(const float* src, int64_t M, int32_t K, int32_t stride, float* dst, void* stream);
/* The same copy, and all of src [M, stride] is zero afterwards (SVOXT_LISTS_GRAD_ZEROED above). */
int svoxt_compact_rows_clear(float* src, int64_t M, int32_t K, int32_t stride, float* dst, void* stream);

/* out: device [Q, 1] = accumulated opacity (alpha). */
int svoxt_opacity_render_fwd(const svoxt_tree* tree, const svoxt_rays* rays,
                             const svoxt_options* opt, float* out, void* stream);

/* grad_out: device [Q, 1].  Same kernel family as volume_render_bwd with zero
 * colour channels (the reference launches render_ray_backward_kernel,
 * rt_kernel.cu:1607): only the sigma column of grad_features is non-zero. */
int svoxt_opacity_render_bwd(const svoxt_tree* tree, const svoxt_rays* rays,
                             const svoxt_options* opt, const float* grad_out,
                             float* grad_features, void* stream);

/* The same pair with sample lists (any thresholds since ABI v20: recorded is every sample with sigma > 0,
 * composited what the forward's thresholds leave): the forward records each ray's
 * samples, the backward walks the lists instead of marching twice and adds the
 * contributions up per 8x8 tile before they go to memory (rec and aux are rewritten:
 * the lists serve one backward).  Every contribution is the reference's
 * delta_t * delta_scale * grad_output * T_ray (rt_kernel.cu:486-490 without colour terms). */
int svoxt_opacity_render_fwd_record(const svoxt_tree* tree, const svoxt_rays* rays, const svoxt_options* opt,
                                    float* out, const svoxt_sample_lists* lists, void* stream);
int svoxt_opacity_render_bwd_replay(const svoxt_tree* tree, const svoxt_rays* rays, const svoxt_options* opt,
                                    const float* grad_out, float* grad_features, int32_t grad_stride,
                                    const svoxt_sample_lists* lists, void* stream);

/* depth: device [Q, 1] = delta_scale * t of the first sample with
 * sigma > sigma_thresh, 0 if none. */
int svoxt_render_depth(const svoxt_tree* tree, const svoxt_rays* rays,
                       const svoxt_options* opt, float* depth, void* stream);

/* Nearest-leaf point query.
 * points  : device [Q, 3] (world coordinates; pass offset=0, scaling=1 for local)
 * values  : device [Q, K]   feature row of the leaf; zeros for an empty leaf
 *           (the reference leaves such rows uninitialised, svox_kernel.cu:282)
 * node_ids: device [Q] int64 packed leaf id node*N^3 + u*N^2 + v*N + w
 * data_ids: device [Q] int64 feature row index, -1 for an empty leaf
 * hit_mask: device [n_internal * N^3] uint8 or NULL; set to 1 for every leaf
 *           slot hit (caller pre-zeroes).  The unique-leaf list the reference
 *           returns as leaf_node is the sorted set of non-zero entries. */
int svoxt_query_fwd(const svoxt_tree* tree, const float* points, int64_t Q,
                    float* values, int64_t* node_ids, int64_t* data_ids,
                    uint8_t* hit_mask, void* stream);

/* Unique-leaf list of a query (the reference's leaf_node, svox_kernel.cu:240-269,
 * 304-320): compacts hit_mask [n_slots] into leaf_node [U, 4] int64 rows
 * (node, u, v, w) in increasing packed-id order and writes U to *count (device).
 * leaf_node must have room for min(Q, n_slots) rows; workspace:
 * svoxt_query_leaves_workspace_bytes(n_slots) device bytes. */
int64_t svoxt_query_leaves_workspace_bytes(int64_t n_slots);
int svoxt_query_leaves(const uint8_t* hit_mask, int64_t n_slots, int32_t N, int64_t* leaf_node,
                       int64_t* count, void* workspace, void* stream);

/* grad_out: device [Q, K]; grad_features: device [M, K], zeroed by this call. */
int svoxt_query_bwd(const svoxt_tree* tree, const float* points, int64_t Q,
                    const float* grad_out, float* grad_features, void* stream);

/* Roofline counters: marches every ray exactly as
 * volume_render_fwd does and adds to counters[5] (device int64, caller
 * pre-zeroes): rays that enter the cube, leaf crossings S, child words read
 * sum(L), crossings with a valid feature index, composited samples. */
int svoxt_count_fwd(const svoxt_tree* tree, const svoxt_rays* rays,
                    const svoxt_options* opt, int64_t* counters, void* stream);

/* Instrumentation for the roofline (no counterpart in the reference): what ONE forward march of
 * this ray batch touches.  row_mask: device [2 * M] bytes, pre-zeroed -- [idx] = 1 for every valid
 * leaf's feature row (read by the forward), [M + idx] = 1 where a sample is composited (read again
 * by the backward).  tree_mask: device bytes, pre-zeroed -- with tree->accel: [cell] for the grid
 * cells and [n_cells + slot] for the (child, data) pairs read; without: [slot] for child words and
 * [n_slots + slot] for data words (N = 2; other N: data words only).  longest: device int64,
 * pre-zeroed <- the most leaf crossings of any ray.  The march is the production one. */
int svoxt_count_touched(const svoxt_tree* tree, const svoxt_rays* rays, const svoxt_options* opt,
                        uint8_t* row_mask, uint8_t* tree_mask, int64_t* longest, void* stream);

/* Instrumentation: counters [2] (device int64, caller-zeroed) or NULL.  While set, the one-kernel
 * per-tile backwards (grad_fused_kernel; grad_wide_kernel for rows of 8 / 16 / 32 floats) add to
 * counters[0] the number of 64-byte atomic requests they send to the gradient table and to counters[1]
 * the number of (tile, window of 16 list positions, feature row) groups they belong to.  Process-wide;
 * meant for bench.py. */
int svoxt_set_bwd_counters(int64_t* counters);

/* Instrumentation (ABI v17): words [32] (device int64, caller-zeroed) or NULL.  While set, the one-kernel
 * per-tile backwards run their CHECKED instances: every index into an LDS array, the lists' block pool
 * and the feature / gradient tables is compared with its extent before it is used; a violation adds one
 * to words[2 + site] (sites: svoxt_bwd_kernels.h, grad_fused_kernel / grad_wide_kernel) and the index is
 * clamped, so the checked run cannot itself leave its arrays; words[31] counts the tiles the checked
 * instances worked on (0: the route taken has no checked instance).  Results are those of the production
 * instances.  Process-wide; meant for tests (the memory fault of round 3). */
int svoxt_set_bwd_check(int64_t* words);
/* (ABI v19) Images of trees with more than `rows` feature rows (M) are walked in super-tiles of 8 x 8 tiles instead of
 * row-major (svoxt_rays.image_width); default 2^21 rows; < 0 restores the default.  Process-wide; a forward that
 * records sample lists and the backward that walks them must run under the same value (tests use 0 to exercise the
 * super-tile walk on small, ragged images).  Returns the value in force before the call. */
int64_t svoxt_set_super_tile_rows(int64_t rows);
/* (ABI v20) The walk the rule above gives this tree / ray batch right now: SVOXT_LISTS_WALK_ROWMAJOR or
 * SVOXT_LISTS_WALK_SUPER for a batch declared an image of 8 x 8 tiles, 0 otherwise (-1: NULL argument).  OR it into
 * svoxt_sample_lists.flags of a recording forward and of the backward over the same lists. */
int32_t svoxt_image_walk(const svoxt_tree* tree, const svoxt_rays* rays);

/* ---- One training step, planned by the library (ABI v21; no counterpart in the reference) -------------------------
 *
 * Everything above is mechanism; WHICH mechanisms a forward + backward pair should use for a payload (sample lists
 * pooled or not, the sigma bitmask and the exponentials table, the forward's hand-over to the backward, march and
 * shade as one launch, the per-tile backward, padded gradient rows) is policy.  These three calls are that policy --
 * the route svox_t_amd's VolumeRenderer takes with every switch at its default -- for hosts that do not want to
 * re-implement it (INTEGRATION.md route C).  Memory stays the caller's: one workspace, sized by the plan.
 *
 *   svoxt_step_plan      host only: decides the route for this tree / batch / options and lays out the workspace.
 *                        pool_blocks: 4 KB list blocks to provide (0: a first guess, 12 per 64-ray tile).  After a
 *                        step, (max over i of step.lists.pool_next[16 i] + 1) * 32 is what the batch used (device
 *                        words; read them whenever convenient): at or above lists.pool_blocks the pool ran dry --
 *                        results are unaffected (such rays march their remainder) but slower; plan the next step
 *                        with more.  A plan stays valid while tree->M / K / N / xform, the batch's shape (Q, image
 *                        size, order given or not), the options' format / basis_dim do not change.
 *   svoxt_step_forward   volume_render (rt_kernel.cu:1362-1379): out [Q, C+1]; leaves in the workspace what the
 *                        backward of the SAME features / rays / options replays.  Thresholds: any (the lists hold
 *                        every sample with sigma > 0).  tree->accel is used if given (build it once per topology);
 *                        tree->sigma_mask / exp_table are ignored -- both are built here, per call, in the workspace.
 *   svoxt_step_backward  volume_render_backward (rt_kernel.cu:1402-1426): grad_features dense [M, K], every element
 *                        written (zero fill included).  Exact arithmetic (every contribution the reference's formula).
 * The workspace must be 256-byte aligned and may be a different allocation for every step (the plan holds offsets),
 * but the backward needs the bytes its forward left.  No call synchronises. */
typedef struct svoxt_step {
    svoxt_sample_lists lists;      /* pointers are (re)bound to the workspace by each call */
    int64_t workspace_bytes;       /* device bytes the two calls need */
    int32_t records;               /* 1: the forward records sample lists and the backward replays them; 0: both march */
    int32_t grad_cols, grad_stride;
    int32_t uses_mask, uses_table;
    int64_t off_mask, off_table, off_tables, tables_bytes, off_rec, off_aux, off_terms, terms_bytes, off_grad_rows,
            off_bwd_ws, bwd_ws_bytes, nt;
    /* a payload one step away from a specialised one is rendered AS it, with dummy channels (one or two channels with a
       basis -> three; RGBA-style rows of 2 .. 31 floats of another width -> 4 / 8 / 16 / 32): zeros in front of sigma and in
       the upstream gradient; the caller sees its own shapes, the same bits */
    int32_t pad_K, pad_real, pad_dummy, pad_w;       /* pad_K == 0: not padded */
    int64_t off_pad_features, off_pad_out, off_pad_gout, off_pad_grad;
} svoxt_step;
int svoxt_step_plan(const svoxt_tree* tree, const svoxt_rays* rays, const svoxt_options* opt, int64_t pool_blocks,
                    svoxt_step* step);
int svoxt_step_forward(const svoxt_tree* tree, const svoxt_rays* rays, const svoxt_options* opt, float* out,
                       svoxt_step* step, void* workspace, void* stream);
int svoxt_step_backward(const svoxt_tree* tree, const svoxt_rays* rays, const svoxt_options* opt, const float* grad_out,
                        float* grad_features, svoxt_step* step, void* workspace, void* stream);

/* Acceleration grid (no counterpart in the reference).  A 2^g x 2^g x 2^g table
 * that caches, per cell, where the root->leaf descent of common.cuh:63-100
 * stands after g levels (the leaf and its data word if it ended earlier), so a
 * march step costs one 4-byte load plus the levels below g instead of a
 * dependent load per level.  Behind the cells the buffer holds one (child word,
 * data word) pair per tree slot, so that the levels below g cost one 8-byte load
 * each and the leaf's data word none.  svoxt_accel_bytes returns the buffer size
 * for a resolution and a tree (4 bytes per cell + 64 bytes per internal node), -1
 * if log2_res is outside [1, 8]; svoxt_accel_build fills `cells` (8-byte aligned) from
 * tree->child / tree->data; trees with 2^27 - 1 feature rows or internal nodes and more
 * are refused (SVOXT_ERR_UNSUPPORTED: a cell has 27 index bits) -- render them without a grid. */
/* (ABI v22) log2_res | SVOXT_ACCEL_BRICKS, g >= 2: the cells lie in bricks of 4 x 4 x 4 (two 128-byte lines) instead of
 * row-major, so that a ray's consecutive crossings and a tile's 64 rays share lines whichever way they point.  It pays
 * where a kernel waits for the cell and nothing else -- the marching wavefronts of the one-launch recording forward of
 * 3-channel payloads: 0.248 -> 0.234 ms at 800 x 800 / depth 8 -- and costs the one-kernel forward, short of issue slots,
 * its six extra integer operations per crossing (0.203 -> 0.216 ms): build the grid a training step renders through in
 * bricks, a grid for forward-only rendering of 3-channel payloads row-major.  Rows of 8 / 16 / 32 floats, whose forward
 * is march + shade as two kernels either way: bricks, and a level finer than the tree's size suggests (depth 9, 578 MB
 * of features, 1024 x 1024: g 7 row-major 0.837 ms forward, g 8 in bricks 0.801).  tree->accel_log2 carries the flag to
 * the kernels; same size. */
#define SVOXT_ACCEL_BRICKS 0x100
int64_t svoxt_accel_bytes(int32_t log2_res, int64_t n_internal);
int     svoxt_accel_build(const svoxt_tree* tree, int32_t log2_res, void* cells, void* stream);

/* Ray ordering for batches that are not images (no counterpart in the reference).  The
 * marching kernels put 64 consecutive rays on one wavefront; a batch in arbitrary order
 * (rays drawn at random from many cameras) then diverges at every step.  svoxt_ray_order
 * writes to perm [Q] (device, int32) the permutation that sorts the batch by the Morton
 * code (7 bits per axis) of the point where each ray enters the tree's cube (rays that miss it last;
 * the order of the rays of one cell is not fixed from run to run): gather
 * origins / dirs / vdirs with it, render the sorted batch through any entry point above and
 * scatter the output rows back -- results are per ray and do not depend on the order.
 * workspace: device, svoxt_ray_order_workspace_bytes(Q) bytes (-1: Q out of range or no
 * device).  Batches declared as images (image_width > 0, camera mode) are refused: they are
 * walked in 8x8 tiles already. */
int64_t svoxt_ray_order_workspace_bytes(int64_t Q);
int     svoxt_ray_order(const svoxt_tree* tree, const svoxt_rays* rays, const svoxt_options* opt,
                        int32_t* perm, void* workspace, int64_t workspace_bytes, void* stream);
/* The gathers and the scatter that go with it: origins / dirs / vdirs [Q, 3] of the sorted batch
 * (row i = row perm[i] of the caller's) in one launch, and rows of `cols` floats either way --
 * scatter = 0: dst[i, :] = src[perm[i], :]; scatter = 1: dst[perm[i], :] = src[i, :]. */
int     svoxt_gather_rays(const svoxt_rays* rays, const int32_t* perm, float* origins, float* dirs, float* vdirs,
                          void* stream);
int     svoxt_permute_rows(const float* src, const int32_t* perm, float* dst, int64_t n, int32_t cols,
                           int32_t scatter, void* stream);

/* Is an undeclared batch a row-major pinhole image (no counterpart in the reference; ABI v22)?  A caller of the
 * reference's API hands over 800 x 800 rays as [640 000, 3] arrays and says nothing; walked in 8 x 8 pixel tiles such a
 * batch needs no sort and its tiles are coherent in direction too.  Two small launches over the first 65 536 rays write
 * result[0 .. 4] (device, int32, room for SVOXT_IMAGE_PROBE_WORDS words: the rest is scratch): [0] 1 if every origin
 * equals the first; [1] how many jumps of the L1 distance between consecutive directions were found (at most 2: a jump
 * is more than four times the median of the first 1 024 distances); [2], [3] their positions; [4] `ticket`, so that a
 * host that reads the words later, from a buffer it reuses, can tell whose answer it holds.  An image of width W has
 * its first jump at W - 1 and its second at 2 W - 1; the caller then sets image_width / image_height (which must be
 * multiples of 8 with W * H = Q).  A hint like every other: results do not depend on what the caller concludes.
 * Q >= 4096; not for camera mode. */
#define SVOXT_IMAGE_PROBE_WORDS 256
int     svoxt_image_probe(const svoxt_rays* rays, int32_t* result, int32_t ticket, void* stream);

/* ---- Octree construction from a point cloud -------------
 *
 * The reference builds a frame's octree by repeating, depth-1 times,
 * `tree[points].refine()` (helpers.py:101-109: a point query, svox_kernel.cu:45-94,
 * its unique-leaf list, :240-324, then N3Tree.refine, svox.py:488-560) on a fresh
 * N = 2 tree, and then `tree.construct_tree(points)` (svox.py:160-161,
 * svox_kernel.cu:110-121: data[leaf of point i] = i).  The two calls below produce
 * the same child / parent_depth / data tables in one pipeline, with one host
 * read in the middle (the node count, to size the tables) instead of one per round:
 * occupancy bitmaps per level instead of repeated descents, integer prefix sums
 * for the node numbering (nodes of a level in increasing packed-parent order,
 * i.e. the order refine() assigns when given the sorted unique-leaf list).
 * Where several points share a finest leaf, the reference keeps whichever thread
 * wrote last; here the smallest point index wins.
 *
 * points          : device [P, 3] fp32, world coordinates
 * offset, scaling : device fp32[3] (as in svoxt_tree)
 * depth           : D in [1, 10]; internal nodes at levels 0..D-1, finest leaf side 2^-D
 * workspace       : svoxt_build_workspace_bytes(depth) device bytes, carried from
 *                   _count to _emit unchanged
 * n_internal      : _count writes the node count to this device int64; _emit takes
 *                   the value the host read back, = rows of the three tables
 * child, data     : device int32 [n_internal, 2, 2, 2]; parent_depth: [n_internal, 2];
 *                   every row is written (no pre-initialisation needed)
 * empty_index     : value for leaf slots that hold no point (any value >= P) */
int64_t svoxt_build_workspace_bytes(int32_t depth);
int svoxt_build_count(const float* points, int64_t P, const float* offset, const float* scaling,
                      int32_t depth, void* workspace, int64_t workspace_bytes,
                      int64_t* n_internal, void* stream);
int svoxt_build_emit(const float* points, int64_t P, const float* offset, const float* scaling,
                     int32_t depth, const void* workspace, int64_t workspace_bytes,
                     int32_t* child, int32_t* data, int32_t* parent_depth,
                     int64_t n_internal, int32_t empty_index, void* stream);

/* N3Tree.refine for an explicit selector (svox.py:520-546; any N): leaf i of
 * leaf_node (device [n_leaves, 4] int64 rows (node, u, v, w), unique, each a leaf
 * slot of a node < filled) becomes internal node filled + i: child[leaf] = offset to
 * it, its N^3 slots inherit the leaf's data word and have child 0, parent_depth =
 * (packed leaf id -- or node_id[i] when node_id is given -- , depth of the leaf's node
 * + 1).  Rows [filled, filled + n_leaves) of the three tables must exist (capacity). */
int svoxt_refine(const int64_t* leaf_node, int64_t n_leaves, int32_t N, int64_t filled, int64_t capacity,
                 int32_t* child, int32_t* data, int32_t* parent_depth, const int32_t* node_id, void* stream);

/* construct_tree (svox.py:160-161, svox_kernel.cu:110-121, 341-352) on an existing
 * tree of any N: data[leaf containing point i] = i; of several points in one
 * leaf the smallest index is kept (the reference: whichever wrote last).
 * tree->data is written; tree->features is not read. */
int svoxt_construct_tree(const svoxt_tree* tree, const float* points, int64_t P, void* stream);

/* ---- Motion variants of the march --------------------------
 *
 * svoxt_motion_render: motion_render (rt_kernel.cu:698-778, 1480-1504).  For each ray,
 * the first sample with sigma > sigma_thresh gives
 *   out       device [Q, J]  distance from the hit point to each of the J = extra_rows
 *                            joint positions extra_data[j][0:3]
 *   depth     device [Q]     t * delta_scale
 *   hit_point device [Q, 3]  (as the reference computes it: transform_coord_world of
 *                            the LEAF-LOCAL coordinates, rt_kernel.cu:745,757)
 *   data_idx  device [Q] int64  feature row of the hit leaf
 * and zeros in all four when nothing is hit. */
int svoxt_motion_render(const svoxt_tree* tree, const svoxt_rays* rays, const svoxt_options* opt,
                        float* out, float* depth, float* hit_point, int64_t* data_idx, void* stream);

/* TreeSpec.joint_features / skinning_weights / joint_index (data_spec.hpp:66-110) */
typedef struct svoxt_motion {
    const float*   joint_features;    /* device [n_joints, feature_dim] */
    int32_t        n_joints;
    int32_t        feature_dim;       /* 1..32 (the reference's fixed tmp_data_dim, rt_kernel.cu:904) */
    const float*   skinning_weights;  /* device [M, n_bind]: weight of each bound joint per feature row */
    const int32_t* joint_index;       /* device [M, n_bind]: which joints; entries outside [0, n_joints) are skipped */
    int32_t        n_bind;
} svoxt_motion;

/* motion_feature_render (rt_kernel.cu:886-981, 1525-1543): out device [Q, feature_dim] =
 * sum_samples weight * sigmoid(sum_j skinning_weight_j * joint_features[joint_index_j]) + T * background
 * (zeros for a ray that misses the cube, :913-919); early stop as volume_render.
 * workspace: svoxt_motion_workspace_bytes(M, feature_dim) device bytes, 16-byte aligned
 * (the per-row blend of the joint features, evaluated once per call; for the backward
 * also the gradient wrt it).  -1 if feature_dim is outside [1, 32]. */
int64_t svoxt_motion_workspace_bytes(int64_t M, int32_t feature_dim);
int svoxt_motion_feature_render_fwd(const svoxt_tree* tree, const svoxt_motion* motion, const svoxt_rays* rays,
                                    const svoxt_options* opt, float* out, void* workspace,
                                    int64_t workspace_bytes, void* stream);

/* Gradient of the above wrt joint_features: grad_joint_features device
 * [n_joints, feature_dim], zeroed by this call.  This is the derivative of the forward
 * (thresholds ignored, as in every backward of the reference); the reference's own
 * motion_feature_render_backward (rt_kernel.cu:983-1061) accumulates into an
 * uninitialised local indexed by bone, so it defines no result to reproduce. */
int svoxt_motion_feature_render_bwd(const svoxt_tree* tree, const svoxt_motion* motion, const svoxt_rays* rays,
                                    const svoxt_options* opt, const float* grad_out,
                                    float* grad_joint_features, void* workspace, int64_t workspace_bytes,
                                    void* stream);

/* ---- Linear blend skinning of points: the producer of transformation_matrices ------
 *
 * warp_vertices (svox_kernel.cu:123-154, 354-378; svox.py:58-76, 974-981):
 *   matrix_out[q]   device [Q, 4, 4] = sum_j (w_qj > 0) w_qj * matrices[joint_qj] on rows 0..2,
 *                   row 3 = (0, 0, 0, 1); 16-byte aligned
 *   vertices_out[q] device [Q, 3]    = matrix_out[q][0:3, 0:3] * points[q] + matrix_out[q][0:3, 3]
 * matrices: device [n_joints, 4, 4]; skinning_weights [Q, n_bind]; joint_index [Q, n_bind] int32
 * (entries outside [0, n_joints) are skipped).  matrix_out is what volume_render takes as
 * svoxt_tree.xform with xform_dim = 4 when rows of `features` are points. */
int svoxt_warp_vertices(const float* matrices, int32_t n_joints, const float* points, int64_t Q,
                        const float* skinning_weights, const int32_t* joint_index, int32_t n_bind,
                        float* vertices_out, float* matrix_out, void* stream);

/* warp_vertices_backward (svox_kernel.cu:156-211, 404-436): from grad_vertices [Q, 3] and
 * grad_matrix_out [Q, 4, 4] to grad_points [Q, 3], grad_matrices [n_joints, 4, 4] (zeroed by
 * this call, float atomics) and grad_skinning_weights [Q, n_bind] (every entry written). */
int svoxt_warp_vertices_bwd(const float* matrices, int32_t n_joints, const float* points, int64_t Q,
                            const float* skinning_weights, const int32_t* joint_index, int32_t n_bind,
                            const float* grad_vertices, const float* grad_matrix_out,
                            float* grad_points, float* grad_matrices, float* grad_skinning_weights,
                            void* stream);

/* ---- Point-to-voxel splat: voxelize (p2v.py:33-54, p2v_kernel.cu:104-286) --------------------------
 *
 * voxels[x][y][z] (device [n, n, n, 1]) = sum over the points p whose window holds (x, y, z) and with
 * r = |xyz_p - (i * voxel_size + volume_corner)| <= conv_radius of
 * expf(-r*r / (2*kernel_radius*kernel_radius)) * point_features[p][F-1], voxel_size = volume_size / (n - 1):
 * the reference's float expressions, so the same (point, voxel) pairs.  Unlike the reference the sum is
 * bit-identical from run to run (no float atomics: points sorted by 4x4x4 tile, one wavefront per tile and
 * chunk of candidates, bins in fixed order and ascending point index within a bin).  Non-finite points
 * contribute nothing.
 *
 * points: device [P, 3]; point_features: device [P, F], F >= 1; volume_corner / volume_size: HOST float[3]
 * (size > 0); n_voxels in [2, 1024]; kernel_radius > 0; conv_radius finite and >= 0; P in [0, 2^31).
 * Every argument is checked before any HIP call (SVOXT_ERR_INVALID).  order (device int32 [P], optional):
 * receives the permutation the forward sorted the points into, for svoxt_p2v_bwd.  workspace: device,
 * svoxt_p2v_workspace_bytes(P, n_voxels, volume_corner, volume_size, conv_radius) bytes, the same arguments as the
 * forward's (-1: invalid arguments, or too many work items: tiles + P x apron bins / 1024 reaches 2^32 -- e.g. P near
 * 2^31 with conv_radius over ~21 voxels; then the forward returns SVOXT_ERR_UNSUPPORTED).  Size: ~40 bytes a point
 * plus ~256 bytes per 1 024 candidates (P x apron bins; 27 bins up to conv_radius = 3 voxels, 125 below 7) plus
 * 12 bytes a tile -- 51 MiB for 1 M points at n = 256 and 2 voxels, 98 GiB for 2^31 - 1 points at 3 voxels.
 * No host read, no synchronisation. */
int64_t svoxt_p2v_workspace_bytes(int64_t P, int32_t n_voxels, const float* volume_corner, const float* volume_size,
                                  float conv_radius);
int svoxt_p2v_fwd(const float* points, const float* point_features, int64_t P, int32_t F,
                  const float* volume_corner, const float* volume_size, int32_t n_voxels,
                  float kernel_radius, float conv_radius, float* voxels, int32_t* order,
                  void* workspace, int64_t workspace_bytes, void* stream);

/* p2v_backward: grad_output device [n, n, n, 1].  points_grad [P, 3] and point_features_grad [P, F]
 * (device, each optional: NULL = not computed) get every element written once, no atomics.  The
 * reference's per-point loop (x -> y -> z) with its expressions and its order of addition per point;
 * the feature gradient goes to column F-1, the column the forward reads (the reference writes column 0,
 * p2v_kernel.cu:203), the other columns are 0.  Non-finite points get zero gradient.  order: the
 * forward's permutation (optional; the walk order only, results do not depend on it). */
int svoxt_p2v_bwd(const float* grad_output, const float* points, const float* point_features, int64_t P,
                  int32_t F, const float* volume_corner, const float* volume_size, int32_t n_voxels,
                  float kernel_radius, float conv_radius, const int32_t* order, float* points_grad,
                  float* point_features_grad, void* stream);

/* ---- Pruning: N3Tree.prune (the halves the reference keeps as tensor ops: merge, svox.py:352-389, and
 * shrink_to_fit, :600-642) ------------------------------------------------------------------------------
 *
 * From the tree tables (child device int32 [>= n_internal, N, N, N], data the same extent, parent_depth device int32
 * [>= n_internal, 2]), the number M of feature rows and a decision per slot of child -- keep (device uint8, non-zero =
 * kept) or weights (device float32; kept iff weights >= threshold, so a NaN weight drops the slot); exactly one of the
 * two, entries at slots that are not leaves are ignored -- the tables of the pruned tree:
 *   1. a leaf (child == 0) that is not kept becomes empty: data = empty_index.  (A leaf is empty when its data word,
 *      read as unsigned, is >= M; a kept empty leaf keeps its word.)
 *   2. collapse != 0: a node other than the root is removed iff no kept, non-empty leaf lies below it; its parent slot
 *      becomes an empty leaf (child 0, data empty_index).  collapse == 0: every node stays.
 *   3. the nodes that stay keep their order and are numbered 0, 1, 2, ...; child words are new_id(child) - new_id(node),
 *      parent_depth[:, 0] is new_id(parent) * N^3 + slot (the root's row is copied), parent_depth[:, 1] is copied,
 *      data at slots that are not leaves is empty_index.
 *   4. compact_features != 0: a feature row stays iff a kept non-empty leaf names it; the rows that stay keep their
 *      order, data is renumbered, row_map (device int64 [new_M]) lists the old row of every new one.
 *      compact_features == 0: data words are left as they are, new_M = M, row_map is not written.
 * Integer work, no order dependence: the outputs are a function of the inputs, identical from run to run.
 *
 * svoxt_prune_count marks and scans; counts (device int64[3]) receives the nodes that stay, the rows that stay and the
 * leaves dropped in step 1.  The host reads it -- the one host read -- allocates child_out / data_out [new_n_internal,
 * N, N, N], parent_depth_out [new_n_internal, 2] and row_map, and calls svoxt_prune_emit with the same inputs and the
 * workspace unchanged; every row of the outputs is written.  workspace: svoxt_prune_workspace_bytes(n_internal, M)
 * device bytes (8 bytes per node and per feature row; -1 for extents outside [1, 2^31) / [0, 2^31)).
 * Every argument is checked before any HIP call (SVOXT_ERR_INVALID): N in [2, 16], n_internal * N^3 < 2^31,
 * empty_index >= M as an unsigned number, no NULL where a pointer is required. */
int64_t svoxt_prune_workspace_bytes(int64_t n_internal, int64_t M);
int svoxt_prune_count(const int32_t* child, const int32_t* data, const int32_t* parent_depth, int64_t n_internal,
                      int32_t N, int64_t M, const uint8_t* keep, const float* weights, float threshold,
                      int32_t collapse, int32_t compact_features, void* workspace, int64_t workspace_bytes,
                      int64_t* counts, void* stream);
int svoxt_prune_emit(const int32_t* child, const int32_t* data, const int32_t* parent_depth, int64_t n_internal,
                     int32_t N, int64_t M, const uint8_t* keep, const float* weights, float threshold,
                     int32_t compact_features, const void* workspace, int64_t workspace_bytes,
                     int64_t new_n_internal, int64_t new_M, int32_t empty_index, int32_t* child_out,
                     int32_t* data_out, int32_t* parent_depth_out, int64_t* row_map, void* stream);

/* dst[i, :] = src[row_map[i], :] for i < n: the feature table (and whatever else is kept per row: optimizer state)
 * behind a prune.  src device float32 [src_rows, cols], dst [n, cols], row_map device int64 [n]; an entry outside
 * [0, src_rows) leaves its row of dst unwritten.  16 bytes a thread when cols is a multiple of 4 and both tables are
 * 16-byte aligned. */
int svoxt_prune_gather_rows(const float* src, int64_t src_rows, const int64_t* row_map, float* dst, int64_t n,
                            int32_t cols, void* stream);

/* ---- Growing: N3Tree.subdivide and N3Tree.unshare (the reference has refine, svox.py:488-560, whose new leaves share
 * the parent's data word) ---------------------------------------------------------------------------------------------
 *
 * subdivide.  From the tree tables (as for svoxt_prune_count), the number M of feature rows and a selection per slot
 * of child -- sel (device uint8, non-zero = selected) or weights (device float32; selected iff weights >= threshold, so
 * a NaN weight never splits), at most one of the two, neither = every slot; entries at slots that are not leaves are
 * ignored.  A slot of a node < n_internal splits iff child == 0, it is selected, parent_depth[node, 1] < depth_limit
 * and its data word, read as unsigned, is < M (split_empty != 0: empty leaves split too).  The splitting slots, in
 * ascending flat order, become the nodes n_internal, n_internal + 1, ...: child[slot] = new id - node, the new node has
 * child 0 everywhere and parent_depth (flat slot index, depth + 1); the split slot's own data word stays as it is.
 *   own_rows == 0: every slot of a new node takes the parent's data word (what svoxt_refine writes); no rows.
 *   own_rows != 0: below a split leaf that names row r, the k-th such leaf in slot order, slot 0 keeps r and slot
 *      j > 0 gets row M + k (N^3 - 1) + (j - 1); below an empty split leaf every slot is empty_index.  row_map (device
 *      int64 [M + rows_added]) lists the old row of every new row: 0 .. M - 1, then each r N^3 - 1 times.
 * Integer work, no order dependence: the outputs are a function of the inputs, identical from run to run.
 *
 * svoxt_subdivide_count marks, scans and lists; counts (device int64[2]) receives the nodes added and the rows added.
 * The host reads it -- the one host read --, makes sure the three tables have n_internal + nodes_added rows (they may
 * be reallocated and copied: the selection is not read again), allocates row_map and calls svoxt_subdivide_emit with
 * the workspace unchanged.  The emit works IN PLACE: it writes the rows [n_internal, n_internal + nodes_added) of the
 * three tables and the child word of every split slot, nothing else.  capacity = the rows the tables have.
 *
 * unshare.  Every leaf slot of a node < n_internal that names a row which a slot with a smaller flat index names too
 * gets a row of its own: rows M, M + 1, ... in ascending slot order; row_map (device int64 [M + rows_added]) as above.
 * svoxt_unshare_count finds the first slot of every row (an integer atomicMin per row), marks and scans; counts
 * (device int64[1]) receives the rows added.  svoxt_unshare_emit rewrites the data words in place and writes row_map.
 *
 * The new feature table (and per-row optimizer state) is svoxt_prune_gather_rows through row_map.
 * workspace: svoxt_subdivide_workspace_bytes(n_internal, N, M) device bytes for either operation (20 bytes per slot;
 * -1 for extents out of range).  Every argument is checked before any HIP call (SVOXT_ERR_INVALID): N in [2, 16],
 * n_internal * N^3 < 2^31, capacity * N^3 < 2^31, M + rows_added < empty_index as an unsigned number, the counts
 * consistent with each other, no NULL where a pointer is required. */
int64_t svoxt_subdivide_workspace_bytes(int64_t n_internal, int32_t N, int64_t M);
int svoxt_subdivide_count(const int32_t* child, const int32_t* data, const int32_t* parent_depth, int64_t n_internal,
                          int32_t N, int64_t M, const uint8_t* sel, const float* weights, float threshold,
                          int32_t depth_limit, int32_t split_empty, int32_t own_rows, void* workspace,
                          int64_t workspace_bytes, int64_t* counts, void* stream);
int svoxt_subdivide_emit(int32_t* child, int32_t* data, int32_t* parent_depth, int64_t n_internal, int32_t N, int64_t M,
                         int64_t capacity, int32_t own_rows, const void* workspace, int64_t workspace_bytes,
                         int64_t nodes_added, int64_t rows_added, int32_t empty_index, int64_t* row_map, void* stream);
int svoxt_unshare_count(const int32_t* child, const int32_t* data, int64_t n_internal, int32_t N, int64_t M,
                        void* workspace, int64_t workspace_bytes, int64_t* counts, void* stream);
int svoxt_unshare_emit(int32_t* data, int64_t n_internal, int32_t N, int64_t M, const void* workspace,
                       int64_t workspace_bytes, int64_t rows_added, int32_t empty_index, int64_t* row_map, void* stream);

/* ---- Dense-grid weights: grid_weights (the reference's grid_weight_render, rt_kernel.cu:1240-1344, 1454-1478) ----
 *
 * Marches rays through a dense density volume sigma (device float32 [R, R, R], cell (u, v, w) at (u R + v) R + w) and
 * keeps per cell the largest compositing weight any ray gave it (weight) and the number of samples taken in it (hits),
 * both device float32 [R, R, R].  One ray: the preamble of the render calls (camera ray and NDC warp as in
 * svoxt_rays / options.ndc_*, p' = offset + scaling p, unit direction, slab test), then while t < tmax: the point
 * origin + t dir, clamped to [0, 1 - 1e-6], times R gives the cell and the cell-local point; delta_t = the cell's
 * chord / R + step_size; if sigma[cell] > sigma_thresh: att = exp(-delta_t delta_scale sigma), w = T (1 - att),
 * T *= att, weight[cell] = max(weight[cell], w), hits[cell] += 1; t += delta_t.  There is no early stop and stop_thresh
 * is not read: of the options only step_size, sigma_thresh and ndc_* are.
 *
 * The maximum is taken on the weight's bit pattern as a signed integer (a negative weight -- possible only with a
 * negative sigma_thresh -- never raises a cell) and the count in integers, converted to float once (exact to 2^24 a
 * cell, where the reference's float adds agree; at most 2^32 - 1 samples a cell and call): neither depends on the order
 * the rays arrive in, so the outputs are bit-identical from run to run.
 *
 * Rays: camera mode (rays->c2w != NULL): n_views >= 1 cameras, c2w_stride (12: [V, 3, 4], 16: [V, 4, 4]) floats apart,
 * sharing fx, fy, image_width and image_height (any size >= 1; walked in 8 x 8 pixel tiles), rays->Q = image_width *
 * image_height; the result is over all n_views * Q rays, one launch.  Ray-batch mode (c2w NULL): origins / dirs device
 * [Q, 3] (vdirs and order are not read), n_views = 1, c2w_stride ignored.
 * offset / scaling: device float32 [3], as svoxt_tree's.  flags: 0 or SVOXT_GRIDW_ACCUMULATE.
 * Every argument is checked before any HIP call (SVOXT_ERR_INVALID): R >= 1 with R^3 < 2^31, step_size finite and > 0
 * (so that every march ends), n_views * tiles < 2^31, no NULL where a pointer is required.  No workspace, no host read,
 * no synchronisation.  While the call's kernels run, hits holds integers: it is a float volume again when they end. */
#define SVOXT_GRIDW_ACCUMULATE 1  /* weight / hits hold an earlier call's result (non-negative integers in hits) and are
                                     updated -- max and count compose across calls; else they are zeroed first */
int svoxt_grid_weights(const float* sigma, int32_t R, const svoxt_rays* rays, int32_t n_views, int32_t c2w_stride,
                       const svoxt_options* opt, const float* offset, const float* scaling, int32_t flags,
                       float* weight, float* hits, void* stream);

/* ---- Palette quantisation: quantize_median_cut (the reference's CPU recursion, svox_t/csrc/quantizer.cpp:48-157) ------
 *
 * Median cut of the rows of data (device float32 [M, K]) into at most 2^order segments, level by level: all rows start
 * as one segment; for `order` levels every segment of more than one row is cut in two, a segment of <= 1 rows is closed
 * and keeps its place.  A cut: the split column is the first one with the largest float32 (max - min); the segment is
 * ordered by (value in that column, row index), -0.0 equal to +0.0; unweighted (weights NULL) the cut is at
 * l + (r - l) / 2, weighted (weights device float32 [M]) at the first position whose inclusive float64 prefix sum of
 * weights is > 0.5 x the segment's total, r if none is; an empty child is a segment like any other.  After the last
 * level the segments, left to right, are the colours 0, 1, ... (the reference's depth-first emission order):
 * color_id_map (device int32 [M]) receives every row's colour, colors (device float32 [2^order, K]) the (weighted)
 * mean of every segment's rows, summed in float64 in a fixed order and rounded once.  Differences from the reference:
 * the row of an empty segment (and every row past the last segment) is zero, not 0 / 0; a non-empty segment whose
 * weights sum to zero takes the plain mean; ties are broken by row index where nth_element / sort leave them open.
 * NaN in data is not checked: the result is then unspecified.  No float atomics: bit-identical from run to run.
 *
 * Checked before any HIP call (SVOXT_ERR_INVALID): order in [0, 16], K >= 1, 2^order <= M < 2^31, no NULL where a
 * pointer is required.  workspace: device, svoxt_quantize_workspace_bytes(M, K, order, weighted) bytes (-1 for
 * arguments outside those limits): ~20 bytes a row (28 weighted) plus 8 K + 24 bytes a colour.  One stream, no host
 * read, no synchronisation. */
int64_t svoxt_quantize_workspace_bytes(int64_t M, int32_t K, int32_t order, int32_t weighted);
int svoxt_quantize_median_cut(const float* data, int64_t M, int32_t K, const float* weights, int32_t order, float* colors,
                              int32_t* color_id_map, void* workspace, int64_t workspace_bytes, void* stream);

/* data_out[i] = map[data_in[i]] where data_in[i], read as unsigned, is < M (a feature row); other words (empty leaves)
 * are copied.  data_in, data_out device int32 [n] (may be the same), map device int32 [M]: a tree's data words through
 * a colour-id map. */
int svoxt_remap_index(const int32_t* data_in, int32_t* data_out, int64_t n, const int32_t* map, int64_t M, void* stream);

/* ---- Frontier reductions and merge: N3Tree.frontier / reduce_frontier / diam_frontier / merge (the reference's tensor
 * ops, svox_t/svox.py:352-483, which read `data` as values; here data names rows of the feature table) -----------------
 *
 * The FRONTIER is the set of nodes other than the root whose N^3 slots are all leaves (child == 0).
 * svoxt_frontier_count flags and scans (child device int32 [>= n_internal, N, N, N]); count (device int64[1]) receives
 * F.  The host reads it -- the one host read -- allocates frontier (device int64 [F]) and calls svoxt_frontier_emit with
 * the workspace unchanged: the ids, ascending.  workspace: svoxt_frontier_workspace_bytes(n_internal) device bytes.
 *
 * svoxt_frontier_reduce: out (device float32 [F, Kc]) row f = op over the children c = 0 .. N^3 - 1 of node nodes[f]
 * (device int64 [F]; any nodes, their slots are read as leaves) of features[data[node, c], cols[j]].  cols: device
 * int32 [n_cols] columns in [0, K) (not checked), or NULL with n_cols = 0 for all K columns (Kc = K).  A child is EMPTY
 * when its data word, read as unsigned, is >= M.  empty_mode SVOXT_EMPTY_ZERO: an empty child counts as a row of zeros;
 * SVOXT_EMPTY_SKIP: only the non-empty children are reduced, a node without one gives zeros.  SUM adds in slot order,
 * sequential float32 (no fused multiply-add); MEAN is that sum divided by the number of children counted (N^3, or the
 * non-empty ones); MAX / MIN take the first child in slot order that attains the extremum (strict comparisons: a NaN
 * never replaces a number).  A node id outside [0, n_internal) gives a row of zeros.
 * svoxt_frontier_reduce_bwd: grad_features (device float32 [M, K], zeroed by the call) receives the gradient of that
 * with respect to features for the upstream grad_out [F, Kc]: SUM / MEAN scatter grad_out (divided by the count) to every
 * non-empty child's row, MAX / MIN to the row of the first child that attains the extremum (nowhere if that child is
 * empty).  Float atomics: bit-reproducible where no element receives more than one term.
 * svoxt_frontier_diam: out (device float32 [F]) = the largest, over pairs of children (under SVOXT_EMPTY_SKIP: of
 * non-empty children), of sqrt(sum_j ((x_a[cols[j]] - x_b[cols[j]]) * scale)^2); 0 without a pair.
 *
 * Merge.  selected (device uint8 [n_internal]): node i is MERGED iff selected[i] != 0 and i is a frontier node.  A
 * merged node is removed and its parent slot becomes a leaf whose word is: the node's data word if all N^3 are equal;
 * the first child's word if all children are empty; otherwise the index of a NEW feature row.  The nodes that stay
 * keep their order and are renumbered as by svoxt_prune_emit (child offsets, parent_depth, empty_index at inner
 * slots).  compact_features != 0: the old rows still named by a leaf are carried, in their order, and renumbered;
 * row_map (device int64 [carried]) lists them.  == 0: all M rows are carried, row_map is not written.  New rows follow
 * the carried ones in ascending id of their merged node; new_row_nodes (device int64 [rows_added]) lists those nodes:
 * the caller fills row carried + i with svoxt_frontier_reduce over new_row_nodes (the tables it reads are the OLD
 * ones).  svoxt_merge_count marks and scans; counts (device int64[3]) = nodes that stay, rows carried, rows added: the
 * one host read.  svoxt_merge_emit, same inputs and the workspace unchanged, writes every row of the outputs.
 * workspace: svoxt_merge_workspace_bytes(n_internal, M) device bytes.  Integer work: the outputs are a function of the
 * inputs, identical from run to run.
 * Every argument of every entry point here is checked before any HIP call (SVOXT_ERR_INVALID): N in [2, 16],
 * n_internal * N^3 < 2^31, M in [0, 2^31), K >= 1, op and empty_mode among the constants, empty_index >= M and >= the
 * new number of rows as an unsigned number, no NULL where a pointer is required. */
#define SVOXT_REDUCE_MEAN 0
#define SVOXT_REDUCE_SUM 1
#define SVOXT_REDUCE_MAX 2
#define SVOXT_REDUCE_MIN 3
#define SVOXT_EMPTY_ZERO 0
#define SVOXT_EMPTY_SKIP 1
int64_t svoxt_frontier_workspace_bytes(int64_t n_internal);
int svoxt_frontier_count(const int32_t* child, int64_t n_internal, int32_t N, void* workspace, int64_t workspace_bytes,
                         int64_t* count, void* stream);
int svoxt_frontier_emit(const void* workspace, int64_t workspace_bytes, int64_t n_internal, int64_t F, int64_t* frontier,
                        void* stream);
int svoxt_frontier_reduce(const float* features, int64_t M, int32_t K, const int32_t* data, int64_t n_internal, int32_t N,
                          const int64_t* nodes, int64_t F, const int32_t* cols, int32_t n_cols, int32_t op,
                          int32_t empty_mode, float* out, void* stream);
int svoxt_frontier_reduce_bwd(const float* features, int64_t M, int32_t K, const int32_t* data, int64_t n_internal,
                              int32_t N, const int64_t* nodes, int64_t F, const int32_t* cols, int32_t n_cols, int32_t op,
                              int32_t empty_mode, const float* grad_out, float* grad_features, void* stream);
int svoxt_frontier_diam(const float* features, int64_t M, int32_t K, const int32_t* data, int64_t n_internal, int32_t N,
                        const int64_t* nodes, int64_t F, const int32_t* cols, int32_t n_cols, int32_t empty_mode,
                        float scale, float* out, void* stream);
int64_t svoxt_merge_workspace_bytes(int64_t n_internal, int64_t M);
int svoxt_merge_count(const int32_t* child, const int32_t* data, const int32_t* parent_depth, int64_t n_internal,
                      int32_t N, int64_t M, const uint8_t* selected, int32_t compact_features, void* workspace,
                      int64_t workspace_bytes, int64_t* counts, void* stream);
int svoxt_merge_emit(const int32_t* child, const int32_t* data, const int32_t* parent_depth, int64_t n_internal,
                     int32_t N, int64_t M, const uint8_t* selected, int32_t compact_features, const void* workspace,
                     int64_t workspace_bytes, int64_t new_n_internal, int64_t carried, int64_t rows_added,
                     int32_t empty_index, int32_t* child_out, int32_t* data_out, int32_t* parent_depth_out,
                     int64_t* row_map, int64_t* new_row_nodes, void* stream);

/* ---- Write and locate leaves by position: N3Tree.set / snap / leaf_boxes (the reference's assign_vertical,
 * svox_kernel.cu:96-108, 326-343, and its _calc_corners, svox.py:808-826) ------------------------------------------------
 *
 * svoxt_assign_leaves: every point (points, device float32 [Q, 3]) is taken to its leaf exactly as by svoxt_query_fwd
 * (tree.offset / tree.scaling, the clamp, the descent); a point whose leaf's data word is not in [0, M) is ignored.
 * The others are grouped by the feature ROW their leaf names -- slots that share a row form one group -- and row r of
 * table (device float32 [tree.M, tree.K], written in place; tree.features is not read) becomes, over the rows q of
 * values (device float32 [Q, K]) of its group:
 *   SVOXT_ASSIGN_LAST   the row of the group's highest point index;
 *   SVOXT_ASSIGN_SUM    acc = values[q0]; acc = acc + values[q] for q1 < q2 < ... : ASCENDING POINT INDEX, sequential
 *                       float32 per column, no fused multiply-add;
 *   SVOXT_ASSIGN_MEAN   that sum divided once by (float)count;
 *   SVOXT_ASSIGN_MAX / _MIN  acc = values[q0]; x > acc ? x : acc (x < acc) in the same order.  Finite values are the
 *                       contract: with a NaN in a group the result is unspecified.
 * Rows without a point are not written.  row_count (device int32 [M], or NULL) is zeroed and receives the number of
 * points of every row.  values must not overlap table.  The outputs are a function of the inputs: two runs give the
 * same bytes.  workspace: svoxt_assign_workspace_bytes(Q, M, reduce) device bytes (-1 for arguments out of range),
 * 4 (Q + M) for LAST, about 21 Q for the others; nothing is allocated by the call, no host read.  Q and M below
 * 2^31 - 1, Q * K below 2^38.  Cost of the sorted modes: a group is reduced by one set of lanes in its fixed order, so
 * a single group of L points takes L dependent steps however small the rest is.
 *
 * svoxt_leaf_corners: corners (device float32 [Q, 3]) = the lower corner in [0, 1]^3 of the slots leaf_node (device
 * int64 [Q, 4]: node, x, y, z), by walking parent_depth (device int32 [>= n_internal, 2]; column 0 = the packed parent
 * slot) to the root: corner = (corner + xyz) / N per level, IEEE divide -- the bits of N3Tree._calc_corners.  A slot
 * out of range, or a walk that does not end within 128 levels, gives NaN.
 * svoxt_snap_points: the descent of svoxt_query_fwd, then that corner, then (corner - tree.offset) / tree.scaling:
 * the lower corner of each point's leaf in the coordinates the points came in.
 * Every argument is checked before any HIP call (SVOXT_ERR_INVALID). */
#define SVOXT_ASSIGN_LAST 0
#define SVOXT_ASSIGN_SUM 1
#define SVOXT_ASSIGN_MEAN 2
#define SVOXT_ASSIGN_MAX 3
#define SVOXT_ASSIGN_MIN 4
int64_t svoxt_assign_workspace_bytes(int64_t Q, int64_t M, int32_t reduce);
int svoxt_assign_leaves(const svoxt_tree* tree, const float* points, int64_t Q, const float* values, int32_t reduce,
                        float* table, int32_t* row_count, void* workspace, int64_t workspace_bytes, void* stream);
int svoxt_leaf_corners(const int32_t* parent_depth, int64_t n_internal, int32_t N, const int64_t* leaf_node, int64_t Q,
                       float* corners, void* stream);
int svoxt_snap_points(const svoxt_tree* tree, const int32_t* parent_depth, const float* points, int64_t Q, float* corners,
                      void* stream);

/* ---- Feature-table optimizers: SGD, RMSprop and Adam as one streaming kernel that can skip untouched rows ------------
 *
 * svoxt_optim_step updates param (device float32 [M, K], in place) from grad (device float32 [M, K], read only) and the
 * kind's state tables (device float32 [M, K] each, in place; svoxt_optim_state_count(kind) of them: 0, 1 or 2, -1 for an
 * unknown kind; a table the kind does not keep is not read and may be NULL).  Everything is float32, element by
 * element, every operation a separate correctly rounded + - * / sqrt, no fused multiply-add, in exactly this order:
 *   SVOXT_OPTIM_SGD           p = p + neg_step * g
 *   SVOXT_OPTIM_SGD_MOMENTUM  b = momentum * b + g;  p = p + neg_step * b                     (b: state1, zero at first)
 *   SVOXT_OPTIM_RMSPROP       v = beta2 * v + one_minus_beta2 * (g * g)
 *                             p = p + neg_step * (g / (sqrt(v) + eps))                        (v: state1; beta2 = alpha)
 *   SVOXT_OPTIM_ADAM          m = m + (g - m) * one_minus_beta1
 *                             v = beta2 * v + one_minus_beta2 * (g * g)
 *                             d = sqrt(v) / bias2_sqrt + eps
 *                             p = p + neg_step * (m / d)                                      (m: state1, v: state2)
 * The scalars of svoxt_optim_hyper are the caller's: each computed in double precision and rounded to float32 once --
 * neg_step = -lr (SGD, RMSprop) or -lr / (1 - beta1^t) (Adam), one_minus_beta1 = 1 - beta1, one_minus_beta2 = 1 - beta2
 * (1 - alpha), bias2_sqrt = sqrt(1 - beta2^t), t the 1-based count of steps taken (global: it advances for every row).
 * This is torch.optim.Adam's form (eps added after the bias correction), not SparseAdam's.  Fields a kind does not name
 * are not read.  There is no weight decay, Nesterov momentum, amsgrad, centered RMSprop or maximize.
 *
 * A row is TOUCHED iff some element of its row of grad compares != 0: +0 and -0 do not touch, a NaN does.  lazy = 1:
 * an untouched row keeps every bit of param and of the state tables, and those are not read for it (the gradient is
 * read once for every row).  lazy = 0: every row is updated -- the moments decay where g = 0, torch.optim's dense
 * semantics.  SVOXT_OPTIM_SGD gives the same table either way.
 * 16 bytes a lane where K % 4 == 0 and every table is 16-byte aligned, 4 bytes otherwise; any K >= 1.  The tables must
 * be distinct and must not overlap.  Checked before any HIP call (SVOXT_ERR_INVALID): kind, M >= 1, K >= 1, M * K < 2^37
 * (indices are 64-bit) and M * G < 2^32 - 256, G the lanes a row takes in the one launch: the power of two >= K / 4 (>= K
 * on the 4-byte path), at most 64 -- K = 28 or 32: M < 2^29; lazy in {0, 1}, no NULL where the kind needs a table, the
 * tables pairwise different.
 * One launch on `stream`; no workspace, no allocation, no host read, no synchronisation.  The result is a function of
 * the inputs: two runs give the same bytes. */
#define SVOXT_OPTIM_SGD 0
#define SVOXT_OPTIM_SGD_MOMENTUM 1
#define SVOXT_OPTIM_RMSPROP 2
#define SVOXT_OPTIM_ADAM 3
typedef struct svoxt_optim_hyper {
    float neg_step;        /* -lr, or -lr / (1 - beta1^t) for Adam */
    float momentum;        /* SGD_MOMENTUM */
    float one_minus_beta1; /* ADAM */
    float beta2;           /* ADAM; RMSPROP: alpha */
    float one_minus_beta2; /* ADAM; RMSPROP: 1 - alpha */
    float bias2_sqrt;      /* ADAM: sqrt(1 - beta2^t) */
    float eps;             /* RMSPROP, ADAM */
} svoxt_optim_hyper;
int svoxt_optim_state_count(int32_t kind);
int svoxt_optim_step(int32_t kind, float* param, const float* grad, float* state1, float* state2, int64_t M, int32_t K,
                     svoxt_optim_hyper hyper, int32_t lazy, void* stream);
/* The damped Newton step on a diagonal curvature (what svoxt_render_hess_rows_* gives), one launch over the table, in
 * place.  Per element, float32, one correctly rounded operation at a time: d = hess + damping; where d > 0.f
 * p = p - lr * (grad / d); otherwise (d <= 0.f, or NaN) the element is not written.  lazy = 1: a row whose grad row is all
 * zeros (the optimizers' TOUCHED rule) is read no further and not written.  param, grad, hess: device float32 [M, K],
 * 4-byte aligned, param distinct from both; M, K >= 1, M * K below 2^37.  Entry point added under ABI v22. */
int svoxt_gauss_newton_step(float* param, const float* grad, const float* hess, int64_t M, int32_t K, float lr, float damping,
                            int32_t lazy, void* stream);

/* ---- Face neighbours of the leaves and the smoothness loss over them: N3Tree.leaf_neighbors / tv / tv_add_grad (not in
 * the reference) ------------------------------------------------------------------------------------------------------
 *
 * The LEAF INDEX of a leaf slot is the number of leaf slots (child == 0) with a smaller flat index among the slots of
 * the nodes below n_internal: its place in the list N3Tree._all_leaves() gives.  Leaf i in node `node` at depth d =
 * parent_depth[node, 1] has the integer CELL COORDINATE c in [0, N^(d + 1))^3: its own slot (x, y, z) is the least
 * significant base-N digit per axis, each ancestor's slot (parent_depth[:, 0], the packed parent slot, walked to the
 * root) the next more significant one.
 *
 * svoxt_leaf_neighbors: neighbors (device int32 [L, 6], columns -x +x -y +y -z +z) row i = for each face the cell t =
 * c +- e_a of the leaf's own level, looked up by ONE descent from node 0: for l = 0 .. d the slot digits are
 * (t / N^(d - l)) mod N; where child[node, slot] == 0 the neighbour is that leaf (of depth l <= d: the same size or
 * coarser) and its leaf index is written, otherwise node += child[node, slot].  -1: t lies outside the cube.  -2: the
 * cell is still a node after level d -- the face is covered by several finer leaves, each of which names leaf i from
 * its side.  A leaf whose depth is outside [0, max_depth], or tables that lead out of range, give -1.  Integer
 * arithmetic only.  L must be the number of leaf slots (the host knows it from the nonzero that lists them).
 * workspace: svoxt_neighbors_workspace_bytes(n_internal, N) device bytes (8 per slot; -1 for arguments out of range).
 * Checked before any HIP call (SVOXT_ERR_INVALID): N in [2, 16]; n_internal >= 1 with n_internal * N^3 < 2^31;
 * max_depth >= 0 with N^(max_depth + 1) < 2^31; L in [0, n_internal * N^3] with 12 L < 2^31; child, parent_depth,
 * neighbors (L > 0) and workspace not NULL; workspace_bytes at least the query's.
 *
 * The EDGE PLAN.  Slot (i, k) of neighbors is an EDGE iff j = neighbors[i, k] >= 0, and depths[j] < depths[i] or the
 * depths are equal and k is odd (every pair of face-adjacent leaves once: from the finer side, at equal sizes from the
 * lower), and both leaves name a feature row (rows, device int64 [L]: the data word where it is in [0, M), anything
 * else -- N3Tree writes -1 -- for an empty leaf), and the two rows differ.  Edge e = 6 i + k yields two INCIDENCES: id
 * 2 e belongs to rows[i] (other row rows[j], sign +), id 2 e + 1 to rows[j] (other row rows[i], sign -).  The plan is
 * a CSR over feature rows: row_ptr (device int32 [M + 1]), other (device int32 [2 E]: of every incidence the other
 * row, each row's incidences in ASCENDING INCIDENCE ID) and meta (device uint8 [2 E]: bit 0 the sign, 1 = -; bits
 * 1 .. 6 depths[i] of the edge's emitting leaf) -- 5 bytes an incidence and 4 a row.
 * svoxt_tv_plan_count marks and scans into marks (svoxt_tv_plan_workspace_bytes(L, -1) device bytes); count (device
 * int64[1]) receives E, the one host read.  svoxt_tv_plan_emit, same inputs and marks unchanged, lists the incidences,
 * sorts them by owning row (a stable radix sort: ids stay ascending within a row) and writes the plan; workspace:
 * svoxt_tv_plan_workspace_bytes(L, E) device bytes (about 36 E; the query gives -1 for L < 0, 12 L >= 2^31 or E > 6 L).
 * Integer work: the plan is a function of the inputs, identical from run to run.
 * Checked before any HIP call (SVOXT_ERR_INVALID), both entry points: L >= 0 with 12 L < 2^31; M in [0, 2^31);
 * neighbors, depths, rows not NULL (L > 0); marks not NULL and marks_bytes at least the query's; count not NULL; emit:
 * E in [0, 6 L], E > 0 only with M >= 2; row_ptr not NULL; with E > 0 other, meta and workspace not NULL and
 * workspace_bytes at least the query's.
 *
 * svoxt_tv_rows: loss = sum over edges of w_e * sum over the selected columns c of rho(f[rows[i], c] - f[rows[j], c]),
 * rho(v) = v * v (p = 2) or |v| (p = 1), w_e = 1 (depth_weights NULL) or depth_weights[depth of leaf i] (device
 * float32 [32]; N3Tree passes N^(-2 (d + 1)), the shared face's area, computed in double and rounded once) -- and
 * G [M, K], its gradient with respect to features (device float32 [M, K]).  One kernel, a lane per (row r, selected
 * column c), lane number r * columns + j; cols: device int32 [n_cols] DISTINCT columns in [0, K) (not checked; a column
 * out of range is skipped), or NULL with n_cols = 0 for all K.  Every operation a separate float32 + - * /, no fused
 * multiply-add, in exactly this order:
 *   a = f[r, c]; g = 0; l = 0; for the row's incidences in ascending id: b = f[other, c]; diff = a - b;
 *     p = 2:  t = w * diff;  g = g + (t + t);  on a + incidence  l = l + t * diff
 *     p = 1:  s = diff > 0 ? 1 : diff < 0 ? -1 : 0;  g = g + s * w;  on a + incidence  l = l + w * |diff|
 * The lanes' l (0 for rows without an incidence and for the lanes behind M * columns) are summed per workgroup of 256
 * consecutive lanes by the tree v[i] = v[i] + v[i + s], s = 128, 64 .. 1; workgroup sums B0, B1, ... are then summed
 * as: u[i] = ((0 + B[i]) + B[i + 256]) + ... for i < 256, the same tree over u; loss = that, divided once by divisor
 * when divisor != 0 (N3Tree: E * columns for reduction = "mean").  Gather only, no atomics: the same bytes in every run.
 *   SVOXT_TV_LOSS        loss (device float32[1]) only; table is not touched;
 *   SVOXT_TV_LOSS_GRAD   and table [M, K] = G: every element written -- g (g / divisor when divisor != 0) at the
 *                        selected columns of rows with an incidence, 0 elsewhere; rows without one are not read;
 *   SVOXT_TV_ACCUMULATE  table[r, c] = table[r, c] + scale * g (one multiply, one add, each rounded) at the selected
 *                        columns of rows with an incidence; everything else keeps its bits; no loss, divisor not read.
 * M = 0 or E = 0: loss = 0, G = 0, nothing accumulated.  workspace (the workgroup sums; not needed by ACCUMULATE):
 * svoxt_tv_workspace_bytes(M, columns) device bytes.  A row shared by many leaves is walked by one lane per column, in
 * its fixed order: a row with J incidences costs J dependent steps.
 * Checked before any HIP call (SVOXT_ERR_INVALID): p in {1, 2}; mode among the constants; M in [0, 2^31); K >= 1;
 * E >= 0 with 2 E < 2^31; cols / n_cols NULL / 0 or not NULL / in [1, K]; M * columns < 2^38; divisor finite and >= 0;
 * scale not NaN; loss not NULL (LOSS, LOSS_GRAD); table not NULL (LOSS_GRAD, ACCUMULATE; M > 0); with M > 0 and E > 0
 * features, row_ptr, other, meta not NULL and, for LOSS / LOSS_GRAD, workspace not NULL and workspace_bytes at least
 * the query's. */
#define SVOXT_TV_LOSS 0
#define SVOXT_TV_LOSS_GRAD 1
#define SVOXT_TV_ACCUMULATE 2
int64_t svoxt_neighbors_workspace_bytes(int64_t n_internal, int32_t N);
int svoxt_leaf_neighbors(const int32_t* child, const int32_t* parent_depth, int64_t n_internal, int32_t N, int32_t max_depth,
                         int64_t L, int32_t* neighbors, void* workspace, int64_t workspace_bytes, void* stream);
int64_t svoxt_tv_plan_workspace_bytes(int64_t L, int64_t E);
int svoxt_tv_plan_count(const int32_t* neighbors, const int32_t* depths, const int64_t* rows, int64_t L, int64_t M, void* marks,
                        int64_t marks_bytes, int64_t* count, void* stream);
int svoxt_tv_plan_emit(const int32_t* neighbors, const int32_t* depths, const int64_t* rows, int64_t L, int64_t M, int64_t E,
                       const void* marks, int64_t marks_bytes, void* workspace, int64_t workspace_bytes, int32_t* row_ptr,
                       int32_t* other, uint8_t* meta, void* stream);
int64_t svoxt_tv_workspace_bytes(int64_t M, int32_t n_cols);
int svoxt_tv_rows(const float* features, int64_t M, int32_t K, const int32_t* row_ptr, const int32_t* other, const uint8_t* meta,
                  int64_t E, const int32_t* cols, int32_t n_cols, int32_t p, const float* depth_weights, float divisor,
                  float scale, int32_t mode, float* loss, float* table, void* workspace, int64_t workspace_bytes, void* stream);

/* ---- depth moments (svoxt_depthmom.hip; not in the reference) --------------------------------------
 * out: device float32 [Q, 3] = {m1, m2, alpha} per ray,
 *     m1 = sum_k w_k z_k    m2 = sum_k w_k z_k^2    alpha = 1 - T_end    w_k = T_k (1 - att_k)
 * over the samples opacity_render composites (sigma > sigma_thresh, until T <= stop_thresh), float32, in this order:
 *     att = exp(-delta_t * delta_scale * sigma);  w = T * (1 - att);
 *     z = delta_scale * t (SVOXT_DEPTH_AT_ENTRY: what svoxt_render_depth reports) or
 *         delta_scale * (t + 0.5 * delta_t) (SVOXT_DEPTH_AT_MID);
 *     m1 += w * z;  m2 += w * (z * z);  T *= att;
 *     T <= stop_thresh: m1 and m2 are multiplied by float(1.0 / (1.0 - double(T))) as the colour forward's channels are,
 *     and the ray ends.
 * A ray that misses the volume gives {0, 0, 0}; the background adds nothing (it has no depth).  With NDC options z is in
 * the space the march runs in, as svoxt_render_depth's is.  Expected depth is m1 / alpha, its variance
 * m2 / alpha - (m1 / alpha)^2.  alpha has the bits of svoxt_opacity_render_fwd.
 * The backward ADDS to grad [M, gstride] (gstride 0: data_dim; the caller zeroes it), column data_dim - 1 only,
 *     delta_t delta_scale (c_k T_{k+1} - sum_{i>k} w_i c_i) + delta_t delta_scale ga T_end,  c_k = g1 z_k + g2 z_k^2
 * for grad_out [Q, 3] rows (g1, g2, ga), by the reference's convention for its backward (rt_kernel.cu:382, 456, 486-490
 * with total_color = c_k): every sample with sigma > 0, no early stop, no rescale, the exponent associated as
 * -delta_t * sigma * delta_scale -- the true gradient at thresholds 0.
 * workspace (optional, both calls): a forward given svoxt_depth_moments_workspace_bytes(Q, max_samples) device bytes
 * (8-byte aligned; 8 bytes + 12 a sample for every ray of the batch rounded up to 64) records up to max_samples
 * (row, delta_t, z) a ray; a backward given the same bytes, the same tree, rays and options reads them instead of
 * marching and marches only behind the end of an over-long ray's records.  A smaller workspace holds as many records a
 * ray as fit; NULL / 0: nothing is recorded, the backward marches (two sweeps).  Every path sums the per-sample values
 * by feature row in LDS per tile of 64 rays and issues one atomic per distinct row and pass.  The result does not
 * depend on the workspace beyond the order of float additions.  No allocation, no synchronisation. */
#define SVOXT_DEPTH_AT_ENTRY 0
#define SVOXT_DEPTH_AT_MID 1
int64_t svoxt_depth_moments_workspace_bytes(int64_t Q, int64_t max_samples);    /* -1: negative argument */
int svoxt_depth_moments_fwd(const svoxt_tree* tree, const svoxt_rays* rays, const svoxt_options* opt, int32_t at,
                            float* out, void* workspace, int64_t workspace_bytes, void* stream);
int svoxt_depth_moments_bwd(const svoxt_tree* tree, const svoxt_rays* rays, const svoxt_options* opt, int32_t at,
                            const float* grad_out, float* grad, int32_t gstride,
                            void* workspace, int64_t workspace_bytes, void* stream);

/* ---- distortion loss (svoxt_distort.hip; not in the reference) -------------------------------------
 * out: device float32 [Q, 2] = {L, alpha} per ray, the distortion loss of mip-NeRF 360 over the ray's leaf crossings,
 *     L = sum_i sum_j w_i w_j |s_i - s_j| + (1/3) sum_i w_i^2 d_i    alpha = 1 - T_end    w_k = T_k (1 - att_k)
 * over the samples opacity_render composites (sigma > sigma_thresh, until T <= stop_thresh), float32, in this order,
 * with A, D, Lb, Lu = 0 and T = 1 at the start:
 *     att = exp(-delta_t * delta_scale * sigma);  w = T * (1 - att);
 *     s = delta_scale * (t + 0.5 * delta_t);  d = delta_t * delta_scale;
 *     not the first sample: D += A * (s - s_previous);          D = sum_{j<k} w_j (s_k - s_j), every addend >= 0
 *     Lb += w * D;  Lu += (w * w) * d;  A += w;  T *= att;
 *     T <= stop_thresh: Lb and Lu are each multiplied twice by float(1.0 / (1.0 - double(T))) -- the moments' rescale,
 *     once per factor of w -- and the ray ends.
 *     L = 2 * Lb + Lu * (1 / 3)
 * A ray that misses the volume gives {0, 0}; the background adds nothing.  s is not normalised to the ray's span; with
 * NDC options it is in the space the march runs in.  alpha has the bits of svoxt_opacity_render_fwd.
 * The backward ADDS to grad [M, gstride] (gstride 0: data_dim; the caller zeroes it), column data_dim - 1 only,
 *     d_k gd (u_k T_{k+1} - sum_{i>k} w_i u_i) + d_k ga T_end
 *     u_k = dL/dw_k = 2 (D_k + E_k) + (2/3) w_k d_k        E_k = sum_{j>k} w_j (s_j - s_k)
 * for grad_out [Q, 2] rows (gd, ga), by the reference's convention for its backward: every sample with sigma > 0, no
 * early stop, no rescale, the exponent associated as -delta_t * sigma * delta_scale -- the true gradient at
 * thresholds 0.  The suffix sum is subtracted down from sum_all w_i u_i = 2 L (L is homogeneous of degree 2 in w).
 * workspace (optional, both calls): as the depth moments' -- a forward given
 * svoxt_distortion_workspace_bytes(Q, max_samples) device bytes (8-byte aligned; 8 bytes + 12 a sample for every ray of
 * the batch rounded up to 64) records up to max_samples (row, delta_t, s) a ray; a backward given the same bytes, the same
 * tree, rays and options reads them instead of marching and marches only behind the end of an over-long ray's records.
 * A smaller workspace holds as many records a ray as fit; NULL / 0: nothing is recorded, the backward marches (two
 * sweeps).  Every path sums the per-sample values by feature row in LDS per tile of 64 rays and issues one atomic per
 * distinct row and pass.  The result does not depend on the workspace beyond the order of float additions.  No
 * allocation, no synchronisation. */
int64_t svoxt_distortion_workspace_bytes(int64_t Q, int64_t max_samples);       /* -1: negative argument */
int svoxt_distortion_fwd(const svoxt_tree* tree, const svoxt_rays* rays, const svoxt_options* opt,
                         float* out, void* workspace, int64_t workspace_bytes, void* stream);
int svoxt_distortion_bwd(const svoxt_tree* tree, const svoxt_rays* rays, const svoxt_options* opt,
                         const float* grad_out, float* grad, int32_t gstride,
                         void* workspace, int64_t workspace_bytes, void* stream);

/* ---- per-sample interface (svoxt_samples.hip; not in the reference) -------------------------------
 * A ray batch's leaf crossings as CSR lists, and the two primitives that turn per-sample values back into per-ray
 * values: march -> samples -> weights from density -> accumulate along rays.
 *
 * A SAMPLE is a leaf crossing of the shared march whose data word names a feature row; with min_sigma (a HOST pointer;
 * NULL: no filter; NaN is refused) only crossings with features[row, data_dim - 1] > *min_sigma -- 0.0 gives the set the
 * backwards walk, sigma > 0.  Rays are walked as every per-ray operator walks them (8 x 8 tiles of a declared image,
 * rays.order, plain batches); the lists come out in ray-index order whatever the walk was.
 *   svoxt_ray_samples_count   marches, scans the per-ray counts and writes offsets int64 [Q + 1] (device, 8-byte
 *                             aligned): ray q's samples are offsets[q] .. offsets[q + 1] - 1, offsets[Q] = T is a 64-bit
 *                             total of its own.  T >= 2^31 has to be refused by the caller after reading offsets[Q]:
 *                             the per-ray starts are 32-bit sums and wrap there, the total does not.
 *                             workspace: svoxt_ray_samples_workspace_bytes(Q) device bytes (8-byte aligned; -1: Q negative
 *                             or 2^31 and more; 0 for Q = 0).
 *   svoxt_ray_samples_emit    marches again with the same arguments and writes, at offsets[q] + k in march order,
 *                             row int32 (the feature row), ray int32 (q), depth float32 = delta_scale * t (the ENTRY z of
 *                             the depth moments) and length float32 = delta_t * delta_scale, each [T].  Nothing is written
 *                             at or behind offsets[q + 1].  No float sum: bit-identical from run to run.
 * The per-sample primitives need no tree.  offsets int64 [Q + 1], Q and T below 2^31; segments are clipped to [0, T).
 *   svoxt_sample_weights_fwd  per ray, in list order, float32 without contraction, T = 1 at the start:
 *                                 sigma > 0:  att = exp(-(length * sigma));  w = T * (1 - att);  T *= att
 *                                 sigma <= 0 (or NaN): w = 0, T unchanged
 *                             w float32 [T], alpha float32 [Q] = 1 - T_end.  No thresholds, no early stop.  With
 *                             sigma = features[row, data_dim - 1] alpha has the bits of svoxt_opacity_render_fwd at
 *                             thresholds 0.
 *   svoxt_sample_weights_bwd  grad_sigma float32 [T] (written, one entry per sample, no atomics) for grad_w [T] and
 *                             grad_alpha [Q] (either may be NULL: zeros):
 *                                 length_k (grad_w_k T_{k+1} - sum_{j>k} grad_w_j w_j + grad_alpha T_end),  0 where sigma <= 0
 *                             in two forward-running sweeps: sweep 1 forms total = sum_j grad_w_j * w_j and T_end; sweep 2
 *                             per sample: total -= grad_w * w;  length * ((grad_w * T_after - total) + grad_alpha * T_end).
 *   svoxt_sample_accumulate_fwd   out float32 [Q, C]: out[q, c] = sum_k w[k] * values[k, c] over the ray's samples,
 *                             acc += w * v in list order.  values float32 [T, C], or NULL with C = 1 (or T = 0): the plain sum of w.
 *   svoxt_sample_accumulate_bwd   one pass over values: grad_w[k] = sum_c grad_out[ray[k], c] * values[k, c] in ascending
 *                             c, grad_values[k, c] = w[k] * grad_out[ray[k], c]; either output may be NULL (not wanted).
 * Q = 0 is a valid no-op everywhere.  No allocation, no synchronisation. */
int64_t svoxt_ray_samples_workspace_bytes(int64_t Q);
int svoxt_ray_samples_count(const svoxt_tree* tree, const svoxt_rays* rays, const svoxt_options* opt, const float* min_sigma,
                            int64_t* offsets, void* workspace, int64_t workspace_bytes, void* stream);
int svoxt_ray_samples_emit(const svoxt_tree* tree, const svoxt_rays* rays, const svoxt_options* opt, const float* min_sigma,
                           const int64_t* offsets, int32_t* row, int32_t* ray, float* depth, float* length, void* stream);
int svoxt_sample_weights_fwd(const int64_t* offsets, int64_t Q, int64_t T, const float* length, const float* sigma, float* w,
                             float* alpha, void* stream);
int svoxt_sample_weights_bwd(const int64_t* offsets, int64_t Q, int64_t T, const float* length, const float* sigma,
                             const float* grad_w, const float* grad_alpha, float* grad_sigma, void* stream);
int svoxt_sample_accumulate_fwd(const int64_t* offsets, int64_t Q, int64_t T, const float* w, const float* values, int32_t C,
                                float* out, void* stream);
int svoxt_sample_accumulate_bwd(const int32_t* ray, int64_t Q, int64_t T, const float* w, const float* values, int32_t C,
                                const float* grad_out, float* grad_w, float* grad_values, void* stream);

/* ---- sample faces and the gradient in the rays (svoxt_samples.hip; not in the reference) -----------
 * The geometric half of a gradient in the rays: how every sample's depth and length move with the ray's origin and
 * direction.  Both ends of a crossing lie on axis-aligned planes -- faces of a leaf, or of the cube for a ray's first
 * crossing --, z = (P_a - o_a) / d_a in the parameter along rays.dirs AS GIVEN (what depth is), so dz/do_a = -1 / d_a and
 * dz/dd_a = -z / d_a, nothing on the other axes.  Only the march knows the axes.  Entry points added under ABI v22.
 *   svoxt_ray_samples_emit_faces   svoxt_ray_samples_emit with a fifth array, face uint8 [T] = entry | exit << 2 (any
 *                             alignment); row / ray / depth / length are svoxt_ray_samples_emit's bit for bit, after the same
 *                             svoxt_ray_samples_count.  In the march's own float32 values:
 *                                 exit    m_a = fmaxf(-l_a * i_a, -l_a * i_a + i_a) on the leaf-local point l and the ray's
 *                                         inverse direction i (the three values whose minimum is the step across the
 *                                         leaf); the first axis in x, y, z (0, 1, 2) that holds min(m_x, m_y, m_z), found
 *                                         by a strict-less update (a NaN never takes over)
 *                                 entry   the exit of the crossing marched immediately before on the same ray, whether that
 *                                         crossing was a sample or not (empty leaves and leaves at or under min_sigma
 *                                         advance it); for the ray's first crossing, with n_a = fminf(t1, t2) of the cube's
 *                                         slab test: tmin > 0: the first axis in x, y, z with n_a == tmin (3 if none);
 *                                         otherwise 3, "no plane" -- the origin lies inside or on the cube and depth does
 *                                         not depend on the ray
 *   svoxt_sample_geometry_bwd      grad_origins / grad_dirs float32 [Q, 3] for grad_depth / grad_length float32 [T] (either may
 *                             be NULL: zeros) and dirs float32 [Q, 3], the direction vectors the lists were marched from.  A
 *                             lane per ray, its segment in list order, float32 without contraction, six accumulators
 *                             go[3] and gd[3] that start at 0; THIS SEQUENCE IS THE DEFINITION.  Per sample k with
 *                             gz_in = grad_depth[k] - grad_length[k] and gz_out = grad_length[k]:
 *                                 a = face & 3;         if a < 3 and d[a] != 0:  u = gz_in / d[a];   go[a] -= u;  gd[a] -= u * depth[k]
 *                                 b = (face >> 2) & 3;  if b < 3 and d[b] != 0:  v = gz_out / d[b];  go[b] -= v;  gd[b] -= v * (depth[k] + length[k])
 *                             the entry term first; depth + length is one float32 add.  Every ray's three and three values
 *                             are written, zeros for a ray without samples.  No atomics: the same bits in every run.
 *                             It is the gradient of the two PLANES.  Two terms of the order of step_size are left out by
 *                             definition: depth of a crossing after a ray's first is its plane's z plus one
 *                             step_size * delta_scale (the previous crossing's overshoot), length holds one more, and
 *                             delta_scale = 1 / |scaling * d| depends on dirs.
 *   svoxt_sample_weights_bwd_length   svoxt_sample_weights_bwd's pass with a second output from the same bracket:
 *                                 grad_length_k = sigma_k ((grad_w_k T_after - total) + grad_alpha T_end),  0 where sigma <= 0
 *                             grad_sigma has svoxt_sample_weights_bwd's bits.  Both outputs are required.
 * Q = 0 is a valid no-op (and T = 0 for svoxt_sample_weights_bwd_length).  No allocation, no synchronisation. */
int svoxt_ray_samples_emit_faces(const svoxt_tree* tree, const svoxt_rays* rays, const svoxt_options* opt, const float* min_sigma,
                                 const int64_t* offsets, int32_t* row, int32_t* ray, float* depth, float* length, uint8_t* face,
                                 void* stream);
int svoxt_sample_geometry_bwd(const int64_t* offsets, int64_t Q, int64_t T, const uint8_t* face, const float* depth, const float* length,
                              const float* dirs, const float* grad_depth, const float* grad_length, float* grad_origins,
                              float* grad_dirs, void* stream);
int svoxt_sample_weights_bwd_length(const int64_t* offsets, int64_t Q, int64_t T, const float* length, const float* sigma,
                                    const float* grad_w, const float* grad_alpha, float* grad_sigma, float* grad_length, void* stream);

/* ---- scans, quantiles and subsets of the lists (svoxt_scan.hip; not in the reference) -------------
 * The conventions of the per-sample primitives above: ray q's segment is max(offsets[q], 0) .. min(offsets[q + 1], T),
 * Q and T below 2^31, float32, sequential in list order without contraction, no float atomic: the same bits in every run.
 *   svoxt_ray_scan_fwd        out float32 [T, C] from values float32 [T, C] (C >= 1), per ray and channel, in list order or,
 *                             with SVOXT_SCAN_REVERSE, from the ray's last sample to its first:
 *                                 acc = 0 | 1 | -inf | +inf                          (SVOXT_SCAN_SUM | PROD | MAX | MIN)
 *                                 new = acc + v | acc * v | (v > acc) ? v : acc | (v < acc) ? v : acc
 *                                 out = new, or with SVOXT_SCAN_EXCLUSIVE acc from before the step;  acc = new
 *                             (max / min never take a NaN; the first occurrence wins a tie).  Elements outside every
 *                             segment are not written.  out must not overlap values.
 *   svoxt_ray_scan_bwd        grad_values float32 [T, C] (every element written: 0 outside the segments; it must overlap
 *                             neither grad_out nor values) for grad_out [T, C].  Positions j = 0 .. n-1 along the scan's
 *                             direction, g = grad_out, v = values (NULL allowed for the sum only):
 *                                 sum    the scan of g with the same EXCLUSIVE and the other direction
 *                                 prod   sweep 1 against the direction:  S_j = g_j + v_{j+1} * S_{j+1},  S_{n-1} = g_{n-1}
 *                                        (EXCLUSIVE: S_j = g_{j+1} + v_{j+1} * S_{j+1},  S_{n-1} = 0);
 *                                        sweep 2 along it, P = 1:  grad_j = P * S_j;  P *= v_j      -- no division: zeros are safe
 *                                 max / min   one sweep along the direction with the running argument a (none at first):
 *                                        inclusive: a moves to j where v_j is taken, then grad_a += g_j; EXCLUSIVE:
 *                                        grad_a += g_j (nowhere while there is no a), then a moves.  Every sum starts at 0
 *                                        and adds in scan order.
 *   svoxt_ray_quantile        per ray and target i < nq (q: device float32 [nq], values in [0, 1] -- the caller's check):
 *                                 c = 0;  per sample with w > 0 (others -- 0, negative, NaN -- are passed over):  c = c + w
 *                                 target = q_i * c_end (normalize != 0) or q_i
 *                                 index[ray, i] = the list index k in [0, T) of the first such sample with c_k >= target,
 *                                 frac[ray, i] = (target - c_{k-1}) / w_k clamped to [0, 1] (NaN: 0);  -1 and 0 where no
 *                                 sample has w > 0 or the target is never reached.
 *                             index int64 [Q, nq] (8-byte aligned), frac float32 [Q, nq].
 *   svoxt_samples_select_*    the samples with keep[k] != 0 (keep: T bytes), in their old order, as new lists:
 *       _workspace_bytes(T)   device bytes (8-byte aligned) shared by the pair; -1: T negative or 2^31 and more; 0 for T = 0
 *       _count                flags, scans (pos = the number of kept samples before each, 32-bit, T + 1 entries) and writes
 *                             offsets_out int64 [Q + 1] = pos[clamped offsets[q]] and total int64 [1] = pos[T] = T'
 *                             (both device, 8-byte aligned).  T = 0: zeros, nothing else is read.
 *       _emit                 with the same keep, T and workspace (unchanged since _count) and T_out = T' read back by the
 *                             caller: ray / row / depth / length of every kept sample copied bit for bit to pos[k], and
 *                             index int64 [T'] = k.  Nothing is written at or behind T_out.
 * Q = 0 and T = 0 are valid no-ops.  No allocation, no synchronisation. */
#define SVOXT_SCAN_SUM 0
#define SVOXT_SCAN_PROD 1
#define SVOXT_SCAN_MAX 2
#define SVOXT_SCAN_MIN 3
#define SVOXT_SCAN_EXCLUSIVE 1
#define SVOXT_SCAN_REVERSE 2
int svoxt_ray_scan_fwd(const int64_t* offsets, int64_t Q, int64_t T, const float* values, int32_t C, int32_t op, int32_t flags,
                       float* out, void* stream);
int svoxt_ray_scan_bwd(const int64_t* offsets, int64_t Q, int64_t T, const float* values, int32_t C, int32_t op, int32_t flags,
                       const float* grad_out, float* grad_values, void* stream);
int svoxt_ray_quantile(const int64_t* offsets, int64_t Q, int64_t T, const float* w, const float* q, int32_t nq, int32_t normalize,
                       int64_t* index, float* frac, void* stream);
int64_t svoxt_samples_select_workspace_bytes(int64_t T);
int svoxt_samples_select_count(const uint8_t* keep, const int64_t* offsets, int64_t Q, int64_t T, int64_t* offsets_out, int64_t* total,
                               void* workspace, int64_t workspace_bytes, void* stream);
int svoxt_samples_select_emit(const uint8_t* keep, int64_t T, const void* workspace, int64_t workspace_bytes, const int32_t* ray,
                              const int32_t* row, const float* depth, const float* length, int64_t T_out, int32_t* ray_out,
                              int32_t* row_out, float* depth_out, float* length_out, int64_t* index, void* stream);

/* ---- new lists out of old ones: split and merge (svoxt_cut.hip; not in the reference) --------------
 * The conventions of the select triple above: a segment is clipped to [0, T), Q and T below 2^31, float32, every operation
 * rounded by itself, no contraction, no float atomic: the same bits in every run.  Each pair is count (one 64-bit total on
 * the device, which the caller reads back and refuses from 2^31 on) and emit.  Entry points added under ABI v22.
 *   svoxt_samples_split_*     every sample k cut into m_k equal pieces, in list order:
 *                                 mf = ceilf(length / max_length)   (pieces == NULL; max_length > 0, +inf allowed), or
 *                                 mf = (float)pieces[k]             (pieces: device int32 [T]; max_length must then be 0)
 *                                 m = 1 where length > 0 is false (0, negative, NaN) or mf >= 1 is false,
 *                                 m = (int)min(mf, (float)max_pieces) otherwise         (max_pieces in [1, 2^30])
 *                                 m == 1: the sample copied bit for bit;  else step = length / (float)m and piece p < m has
 *                                 depth + (float)p * step and length step.  Every piece keeps ray and row.
 *       _workspace_bytes(T)   device bytes (8-byte aligned) shared by the pair; -1: T negative or 2^31 and more; 0 for T = 0
 *       _count                pos = the number of pieces before each sample (32-bit scan over T + 1 entries),
 *                             offsets_out int64 [Q + 1] = pos[clamped offsets[q]], total int64 [1] = the 64-bit sum of m
 *                             (both device, 8-byte aligned; offsets_out means nothing where total >= 2^32).  T = 0: zeros.
 *       _emit                 with the same T and workspace (unchanged since _count) and T_out = total: a lane per piece j
 *                             finds its source k by a binary search in pos and writes ray / row / depth / length and
 *                             index int64 [T_out] = k.  Nothing is written at or behind T_out.
 *   svoxt_samples_merge_*     the union of two lists of the SAME Q rays (depth along the same direction vectors): per ray the
 *                             pieces between all breakpoints of both lists that at least one list covers, with the index of
 *                             the covering sample of each list (-1: none).  A sample is [s, e), s = depth, e = depth + length
 *                             (one float32 add); each list has a current sample and a cursor c that starts at its s.  Until
 *                             both lists are exhausted, the first rule that applies:
 *                               1. a current sample with e > s false (length 0, negative, NaN; NaN depth) is emitted whole and
 *                                  alone: (s, length, its index, -1); A's before B's.  That list advances.
 *                               2. B exhausted or e_a <= c_b: A alone from c_a, length = A's length if c_a == s_a else
 *                                  e_a - c_a.  A advances.
 *                               3. A exhausted or e_b <= c_a: the same for B.
 *                               4. c_a < c_b: A alone, (c_a, c_b - c_a); c_a = c_b.
 *                               5. c_b < c_a: B alone, (c_b, c_a - c_b); c_b = c_a.
 *                               6. c_a == c_b: hi = min(e_a, e_b); both indices, depth c_a, length = A's length if c_a == s_a
 *                                  and hi == e_a, else B's length if c_b == s_b and hi == e_b, else hi - c_a;
 *                                  c_a = c_b = hi; each list with e <= hi advances.
 *                             A ray has at most 2 (n_a + n_b) pieces; merging with an empty list, or a list of samples with
 *                             e > s with itself, returns the list bit for bit.  Samples outside every segment take no part.
 *       _workspace_bytes(Q)   device bytes (8-byte aligned) of _count; -1: Q negative or 2^31 and more; 0 for Q = 0
 *       _count                walks every ray once; offsets_out int64 [Q + 1] (offsets_out[Q] = total) and total int64 [1],
 *                             the 64-bit number of pieces.  Arrays of a list with T = 0 may be NULL (offsets not).
 *       _emit                 walks again and writes ray (= q), row (= -1), depth, length, index_a, index_b int64 at
 *                             offsets_out[q] ..; never at or behind min(offsets_out[q + 1], T_out).
 * No allocation, no synchronisation. */
int64_t svoxt_samples_split_workspace_bytes(int64_t T);
int svoxt_samples_split_count(const float* length, const int32_t* pieces, float max_length, int32_t max_pieces, const int64_t* offsets,
                              int64_t Q, int64_t T, int64_t* offsets_out, int64_t* total, void* workspace, int64_t workspace_bytes,
                              void* stream);
int svoxt_samples_split_emit(int64_t T, const void* workspace, int64_t workspace_bytes, const int32_t* ray, const int32_t* row,
                             const float* depth, const float* length, int64_t T_out, int32_t* ray_out, int32_t* row_out,
                             float* depth_out, float* length_out, int64_t* index, void* stream);
int64_t svoxt_samples_merge_workspace_bytes(int64_t Q);
int svoxt_samples_merge_count(const int64_t* offsets_a, const float* depth_a, const float* length_a, int64_t T_a, const int64_t* offsets_b,
                              const float* depth_b, const float* length_b, int64_t T_b, int64_t Q, int64_t* offsets_out, int64_t* total,
                              void* workspace, int64_t workspace_bytes, void* stream);
int svoxt_samples_merge_emit(const int64_t* offsets_a, const float* depth_a, const float* length_a, int64_t T_a, const int64_t* offsets_b,
                             const float* depth_b, const float* length_b, int64_t T_b, int64_t Q, const int64_t* offsets_out, int64_t T_out,
                             int32_t* ray_out, int32_t* row_out, float* depth_out, float* length_out, int64_t* index_a, int64_t* index_b,
                             void* stream);

/* ---- samples to feature rows and back (svoxt_rows.hip; not in the reference) ----------------------
 * The row side of the per-sample interface: a gather of table rows by sample, and its inverse, a reduction of
 * per-sample values by feature row over a fixed-order plan.  Gather only: no atomics on floats anywhere, every result
 * bit-identical from run to run.  Entry points added under ABI v22.
 *
 * THE ROW PLAN inverts row int32 [T] (svoxt_ray_samples_emit's, or any other): for every feature row r < M the samples
 * that name it, in ascending sample index.  key = row where 0 <= row < M, M for anything else: samples whose row lies
 * outside [0, M) are not an error, they sort behind row_ptr[M] and take no part in anything.
 *   row_ptr  int32 [M + 1]   row r's samples are perm[row_ptr[r]] .. perm[row_ptr[r + 1] - 1]
 *   perm     int32 [T]       the sample indices sorted stably by key
 *   info     int64 [4]       n_outside = T - row_ptr[M];  the longest segment;  n_long, the rows with more than
 *                            SVOXT_ROW_CHUNK samples;  n_chunks, the sum of ceil(n / SVOXT_ROW_CHUNK) over them
 *   svoxt_row_plan_build   writes the three (all device; info 8-byte aligned): key -> stable LSD radix sort over the bits
 *                          of M -> a binary search per row -> per-row marks and two scans.  The caller reads info (the one
 *                          host read).  workspace: svoxt_row_plan_workspace_bytes(T, M) device bytes (-1: T or M negative
 *                          or 2^31 and more; 0 for T = 0), 4-byte aligned.  T = 0: row_ptr and info are zeroed, the
 *                          workspace is not needed.
 *                          Checked before any HIP call, in this order: T, M in [0, 2^31); row_ptr, info not NULL; with
 *                          T > 0 row, perm not NULL; alignment (row / row_ptr / perm 4 bytes, info 8); with T > 0 the
 *                          workspace: alignment, not NULL, at least the query's size.
 *   svoxt_row_plan_long    with info's n_long and n_chunks and the SAME workspace, unchanged since the build: writes
 *                          long_rows int32 [n_long] (ascending), long_chunk_ptr int32 [n_long + 1] (the first chunk of
 *                          every long row; [n_long] = n_chunks) and chunk_long int32 [n_chunks] (the index into
 *                          long_rows of every chunk).  n_long = 0: long_chunk_ptr[0] = 0, the workspace is not read.
 *                          Checked: T, M; n_long in [0, min(M, T / (SVOXT_ROW_CHUNK + 1))]; n_chunks in
 *                          [2 n_long, T / SVOXT_ROW_CHUNK + n_long]; long_chunk_ptr not NULL; with n_long > 0 row_ptr,
 *                          long_rows, chunk_long not NULL; alignment (4 bytes); with n_long > 0 the workspace as above.
 *
 *   svoxt_gather_rows      out float32 [T, C]: out[k, j] = table[row[k], cols[j]] (cols int32 [n_cols] distinct columns,
 *                          or NULL / 0: all K, C = K).  A sample whose row is outside [0, M) gets zeros and the table is
 *                          not read for it.  One kernel; 16 bytes per lane where all columns are taken, K is a multiple
 *                          of 4 and table and out are 16-byte aligned.  T = 0: a no-op.
 *                          Checked: T, M; K >= 1; cols / n_cols NULL / 0 or n_cols in [1, K]; T * C and M * K below
 *                          2^38; with T > 0: row, out not NULL, table not NULL when M > 0, alignment (4 bytes).
 *
 *   svoxt_reduce_rows      out float32 [M, K] from values float32 [T, C] over a plan.  Without cols (NULL / 0) C = K and
 *                          out[r, c] is the reduction of column c; with cols C = n_cols, out[r, cols[j]] is the
 *                          reduction of column j and every other element of out is 0: every element written (the
 *                          gradient of svoxt_gather_rows with respect to the table is this with op = SVOXT_ROWS_SUM).
 *                          The order below is part of the definition.  Every operation is a separate float32 operation
 *                          without contraction.  For row r with the n samples k_0 < k_1 < ... < k_{n-1}
 *                          (perm[row_ptr[r] : row_ptr[r + 1]]) and column c:
 *                            sum         chunk j covers k_{256 j} ... k_{min(256 j + 255, n - 1)}.  The chunk's partial is
 *                                        p_j = ((0 + v[k_first]) + v[k_next]) + ... in ascending order.  The row's value
 *                                        is (p_0 + p_1) + p_2 + ... in ascending j.  With n <= 256 this is the plain
 *                                        sequential sum.
 *                            mean        that sum, divided once by (float) n.
 *                            max / min   the largest or smallest value, NaN as soon as any value of the row is NaN.
 *                            n = 0       `empty`, for every op.
 *                          (256 is SVOXT_ROW_CHUNK.)  A lane per (row, column) for the rows of at most 256 samples; for
 *                          the long rows a lane per (chunk, column) writes partials to the workspace and a lane per
 *                          (long row, column) joins them.  workspace: svoxt_reduce_rows_workspace_bytes(n_chunks, C)
 *                          device bytes (-1: n_chunks negative or 2^31 and more, C < 1, n_chunks * C from 2^38; 0 for
 *                          n_chunks = 0), 4-byte aligned.  M = 0: a no-op; T = 0: `empty` everywhere (cols: at the
 *                          selected columns).
 *                          Checked: T, M; C, K >= 1; cols / n_cols; C = n_cols (or K without cols); op among the
 *                          constants; T * C and M * K below 2^38; n_long and n_chunks as above; with M > 0: out, row_ptr
 *                          not NULL; with T > 0 values, perm not NULL; with n_long > 0 long_rows, long_chunk_ptr,
 *                          chunk_long not NULL; alignment (4 bytes); with n_long > 0 the workspace not NULL and at least
 *                          the query's size.  `empty` may be anything.
 * No allocation, no synchronisation. */
#define SVOXT_ROW_CHUNK 256
#define SVOXT_ROWS_SUM 0
#define SVOXT_ROWS_MEAN 1
#define SVOXT_ROWS_MAX 2
#define SVOXT_ROWS_MIN 3
int64_t svoxt_row_plan_workspace_bytes(int64_t T, int64_t M);
int svoxt_row_plan_build(const int32_t* row, int64_t T, int64_t M, int32_t* row_ptr, int32_t* perm, int64_t* info,
                         void* workspace, int64_t workspace_bytes, void* stream);
int svoxt_row_plan_long(const int32_t* row_ptr, int64_t T, int64_t M, int64_t n_long, int64_t n_chunks,
                        const void* workspace, int64_t workspace_bytes, int32_t* long_rows, int32_t* long_chunk_ptr,
                        int32_t* chunk_long, void* stream);
int svoxt_gather_rows(const float* table, int64_t M, int32_t K, const int32_t* row, int64_t T, const int32_t* cols,
                      int32_t n_cols, float* out, void* stream);
int64_t svoxt_reduce_rows_workspace_bytes(int64_t n_chunks, int32_t C);
int svoxt_reduce_rows(const float* values, int64_t T, int32_t C, const int32_t* row_ptr, const int32_t* perm, int64_t M,
                      const int32_t* long_rows, const int32_t* long_chunk_ptr, const int32_t* chunk_long, int64_t n_long,
                      int64_t n_chunks, const int32_t* cols, int32_t n_cols, int32_t K, int32_t op, float empty,
                      float* out, void* workspace, int64_t workspace_bytes, void* stream);

/* ---- The deterministic render backward: sums by the row plan, not atomics (not in the reference) ------
 * The gradient of svoxt_volume_render_fwd / svoxt_opacity_render_fwd with respect to the feature table,
 *   grad[r, j] = the sum, over the samples that name row r, of the sample's contribution to column j,
 * the same function of (tree, features, rays in index order, options, grad_out) in every run: it does not depend on the
 * assignment of rays to lanes (rays.order, the image hint), on a pool or a previous call, or on the device's size.
 *   The samples      the leaf crossings with a feature row and sigma > 0.f: no threshold, no early stop, whatever the
 *                    options say (the convention of svoxt_volume_render_bwd).
 *   A contribution   float32, no contraction, the operations of the reference's trace_ray_backward (rt_kernel.cu:331-496)
 *                    one by one: att = expf(-delta_t * sigma * delta_scale); weight = light * (1 - att); per channel c
 *                    tmp = sum over i = min_comp .. max_comp of basis[i] * row[c * basis_dim + i] from 0.f (RGBA: row[c]),
 *                    sig = (float)(1.0 / (1.0 + (double)expf(-tmp))), gsig = (float)((double)sig * (1.0 - (double)sig));
 *                    colour column (c, i): weight * basis[i] * gsig * g[c]  (RGBA column j: weight * sig * (1.f - sig) *
 *                    g[j]); sigma column: delta_t * delta_scale * (total_color * light - accum) + delta_t * delta_scale *
 *                    g[C] * light_ray, accum and total_color as the reference's two passes form them.
 *   The order        svoxt_reduce_rows' rule, word for word: a row's samples run in ascending sample index (ray index
 *                    first, then march order within the ray); chunks of SVOXT_ROW_CHUNK = 256 are each added sequentially
 *                    from 0.f; the chunk partials are added in chunk order.
 *   Every element of grad [M, K] is written: the caller need not clear it.  Columns outside [min_comp, max_comp] of a
 *   channel, columns between C * basis_dim and K - 1, and rows no sample names are exactly 0.f.  With a row stride
 *   above K the floats between the rows are not touched.
 * grad_out is float32 [Q, grad_cols], grad_cols = C + 1 = svoxt_out_data_dim, or 1: the opacity backward (C = 0).
 * tree.xform (transformation_matrices) is not served: SVOXT_ERR_INVALID.  The five steps, in this order, each on `stream`:
 *   svoxt_render_grad_rows_count    offsets int64 [Q + 1] (device) of the sample lists: svoxt_ray_samples_count with
 *                                   min_sigma = 0 and its workspace, svoxt_ray_samples_workspace_bytes(Q).  The caller
 *                                   reads T = offsets[Q] (the one host read; from 2^31 on: split the batch).
 *   svoxt_render_grad_rows_emit     marches again and leaves per sample row, ray and delta_t, per ray its basis values
 *                                   and delta_scale, in the workspace: svoxt_render_grad_rows_workspace_bytes(Q, T, M, K,
 *                                   C, basis_dim) device bytes, 8-byte aligned, the same workspace for every step
 *                                   (basis_dim: the options' for SH / SG / ASG with C > 0, else 0; -1: an argument
 *                                   negative or from 2^31, K < 1, C outside [0, K), basis_dim above 25, T * (C + 1) or
 *                                   M * K from 2^38; 0 for T = 0).  Per sample it holds 4 * (C + 4) bytes (row, ray,
 *                                   weight, the sigma contribution, C channel values) and the plan's perm, per ray
 *                                   basis_dim + 1 floats, the plan's own arrays and svoxt_row_plan_build's workspace.
 *                                   No [T, K] array exists at any point.
 *   svoxt_render_grad_rows_plan     svoxt_row_plan_build over the emitted rows; info int64 [4] (device) as there: the
 *                                   caller reads n_long = info[2] and n_chunks = info[3] (the plan's one host read).
 *   svoxt_render_grad_rows_sweep    AFTER the plan and ONCE per emit (it overwrites row, delta_t and what the plan's sort
 *                                   left behind: a plan built after it, or a second sweep, gives wrong sums silently): a lane per (sample, channel) shades, a lane per sample
 *                                   forms its total_color the two ways the reference's passes do, a lane per ray runs the
 *                                   two passes; leaves per sample the weight, the sigma contribution and per channel gsig
 *                                   (RGBA: sig).  It may be queued before info is read.
 *   svoxt_render_grad_rows_reduce   after the sweep: svoxt_row_plan_long, then a lane per (row, column) sums the row's
 *                                   contributions, formed on the fly, into grad (row stride grad_stride floats, 0: K).
 *                                   T = 0: zeros, the workspace may be NULL and no other step is needed.
 * Checked: the tree, rays and options as svoxt_volume_render_bwd checks them; tree.xform NULL; Q, M, T below 2^31;
 * grad_cols >= 1 and, above 1, equal to svoxt_out_data_dim; offsets / grad_out not NULL with Q > 0; info / grad not NULL;
 * grad_stride 0 or >= K; n_long / n_chunks as svoxt_row_plan_long; the workspace's size.  No allocation, no
 * synchronisation. */
int64_t svoxt_render_grad_rows_workspace_bytes(int64_t Q, int64_t T, int64_t M, int32_t K, int32_t C, int32_t basis_dim);
int svoxt_render_grad_rows_count(const svoxt_tree* tree, const svoxt_rays* rays, const svoxt_options* opt, int64_t* offsets,
                                 void* workspace, int64_t workspace_bytes, void* stream);
int svoxt_render_grad_rows_emit(const svoxt_tree* tree, const svoxt_rays* rays, const svoxt_options* opt,
                                const int64_t* offsets, int64_t T, const float* grad_out, int32_t grad_cols,
                                void* workspace, int64_t workspace_bytes, void* stream);
int svoxt_render_grad_rows_plan(const svoxt_tree* tree, const svoxt_rays* rays, const svoxt_options* opt,
                                const int64_t* offsets, int64_t T, const float* grad_out, int32_t grad_cols, int64_t* info,
                                void* workspace, int64_t workspace_bytes, void* stream);
int svoxt_render_grad_rows_sweep(const svoxt_tree* tree, const svoxt_rays* rays, const svoxt_options* opt,
                                 const int64_t* offsets, int64_t T, const float* grad_out, int32_t grad_cols,
                                 void* workspace, int64_t workspace_bytes, void* stream);
int svoxt_render_grad_rows_reduce(const svoxt_tree* tree, const svoxt_rays* rays, const svoxt_options* opt,
                                  const int64_t* offsets, int64_t T, const float* grad_out, int32_t grad_cols,
                                  int64_t n_long, int64_t n_chunks, float* grad, int32_t grad_stride, void* workspace,
                                  int64_t workspace_bytes, void* stream);

/* ---- se_grad: the gradient and a Gauss-Newton diagonal in one pass (not in the reference) ------
 * Next to grad [M, K] -- THE BITS svoxt_render_grad_rows_* gives for the same grad_out -- a second table
 *   hess[m, j] = the sum, over the samples k that name row m and the outputs c, of curv[ray(k), c] * J(k, c, j)^2,
 * J(k, c, j) the derivative of out[ray(k), c] with respect to entry j of row m THROUGH SAMPLE k ALONE, curv float32
 * [Q, grad_cols] the second derivative of a per-pixel separable loss in each output (for squared error: the coefficient of
 * the residual).  The squares are per sample: this is the exact diagonal of the Gauss-Newton Hessian whenever no ray names
 * a row twice, and the svox family's approximation (the squares of a row's samples on one ray are summed, their cross
 * terms dropped) where rows are shared -- after refine, merge, quantize.  Entry points added under ABI v22.
 *   The samples and conventions are the deterministic backward's: crossings with a row and sigma > 0.f; thresholds 0, no
 *   early stop; att = pexpf(-delta_t * sigma * delta_scale); sig = (float)(1.0 / (1.0 + (double)e)); gsig through double;
 *   everything float32 without contraction.  Per sample k of ray q, h its entry at column j:
 *   Colour column j = c * basis_dim + i, min_comp <= i <= max_comp:
 *     jac = weight * basis[q, i] * gsig[k, c]   (RGBA rows: jac = weight * sig * (1.f - sig)), left to right, the prefix
 *     of the gradient's contribution; h = (jac * jac) * curv[q, c].  Only channel c depends on that column.
 *   Sigma column (j = K - 1): h starts at 0.f.  For c = 0 .. C - 1 ascending, a per-channel two-pass walk of the ray's list:
 *     pass 1: accum_c = the sum of weight_k * sig[k, c] in list order from 0.f (light = 1.f; weight = light * (1.f - att);
 *             light *= att), then accum_c += light_ray * background_brightness;
 *     pass 2, from light = 1.f: weight = light * (1.f - att); light *= att; accum_c -= weight * sig[k, c];
 *             jac = (delta_t * delta_scale) * (sig[k, c] * light - accum_c); h += (jac * jac) * curv[q, c].
 *     Last, the alpha channel: jac = (delta_t * delta_scale) * light_ray; h += (jac * jac) * curv[q, C].
 *   Any other column, and columns outside [min_comp, max_comp]: exactly 0.f.  Rows no sample names: exactly 0.f.  Every
 *   element of hess is written; with a row stride above K the padding is untouched.
 *   The sum over a row follows svoxt_reduce_rows' order rule: samples in ascending index, chunks of SVOXT_ROW_CHUNK = 256
 *   from 0.f, the partials in chunk order, rows of more than 256 samples by the long-row path.
 * The steps: svoxt_render_grad_rows_count, _emit and _plan as they are, over a workspace of
 * svoxt_render_hess_rows_workspace_bytes(Q, T, M, K, C, basis_dim) bytes (the gradient's, one float a sample for the sigma
 * entry and a transient [T, C] for sig; -1 and 0 as the gradient's query), then
 *   svoxt_render_hess_rows_sweep    in the place of svoxt_render_grad_rows_sweep, AFTER the plan and ONCE per emit: the
 *                                   gradient's kernels, and between its shade and its totals a lane per (sample, channel)
 *                                   for sig, a lane per (ray, output) for the per-channel walks, a lane per sample for the
 *                                   sum over the outputs.
 *   svoxt_render_hess_rows_reduce   svoxt_render_grad_rows_reduce into grad, then the same plan over the squares into
 *                                   hess (row stride hess_stride floats, 0: K).  T = 0: zeros in both.
 * Checked: what svoxt_render_grad_rows_* checks (tree.xform NULL; Q, M, T below 2^31; T (C + 1) and M K below 2^38;
 * grad_cols = 1, C = 0, is served); curv not NULL with Q > 0, 4-byte aligned; hess not NULL, distinct from grad,
 * hess_stride 0 or >= K; the workspace's size.  No allocation, no synchronisation, no float atomic. */
int64_t svoxt_render_hess_rows_workspace_bytes(int64_t Q, int64_t T, int64_t M, int32_t K, int32_t C, int32_t basis_dim);
int svoxt_render_hess_rows_sweep(const svoxt_tree* tree, const svoxt_rays* rays, const svoxt_options* opt,
                                 const int64_t* offsets, int64_t T, const float* grad_out, const float* curv,
                                 int32_t grad_cols, void* workspace, int64_t workspace_bytes, void* stream);
int svoxt_render_hess_rows_reduce(const svoxt_tree* tree, const svoxt_rays* rays, const svoxt_options* opt,
                                  const int64_t* offsets, int64_t T, const float* grad_out, const float* curv,
                                  int32_t grad_cols, int64_t n_long, int64_t n_chunks, float* grad, int32_t grad_stride,
                                  float* hess, int32_t hess_stride, void* workspace, int64_t workspace_bytes, void* stream);

/* ---- shade_samples: per-sample colours from feature rows (svoxt_shade.hip; not in the reference) ----
 * The shading step of the per-sample interface: the basis of a sample's ray dotted into its feature row's coefficients,
 * then the sigmoid -- and the gradient with respect to the feature table, summed over the row plan.  No [T, K] array
 * exists at any point, no float atomic, every result bit-identical from run to run.  Entry points added under ABI v22.
 *
 *   svoxt_view_basis          basis float32 [Q, basis_dim]: the ray's basis values exactly as the render kernels form them
 *                             from the view direction (rays.vdirs[q], or the pixel's direction in camera mode): SH 1 / 4 /
 *                             9 / 16 / 25 in closed form, SG / ASG from tree.extra_data.  Components outside [min_comp,
 *                             max_comp] are still written: the basis does not depend on the range.  RGBA (and Q = 0): a
 *                             no-op, basis may be NULL.  A lane per ray, no march; rays.order and the image hint are not
 *                             consulted.  Checked: the tree, rays and options as svoxt_volume_render_fwd checks them;
 *                             tree.xform NULL; Q below 2^31; basis not NULL, 4-byte aligned.
 *
 *   svoxt_shade_samples_fwd   values float32 [T, C] and sigma float32 [T] for the samples (row int32 [T], ray int32 [T]) of
 *                             a table features float32 [M, K].  C = svoxt_out_data_dim - 1: K - 1 for RGBA, (K - 1) /
 *                             basis_dim otherwise.  basis is svoxt_view_basis' [Q, basis_dim] (RGBA: not read, may be
 *                             NULL, as ray).  The definition is fixed operation for operation, in float32 without
 *                             contraction.  For sample k with row r and ray q:
 *                               tmp          = sum over i = min_comp .. max_comp of basis[q, i] * features[r, c * basis_dim
 *                                              + i], summed from 0.f in ascending i.  For RGBA, tmp = features[r, c].
 *                               values[k, c] = (float)(1.0 / (1.0 + (double)expf(-tmp))) with activate != 0 (expf: the
 *                                              library's fixed operation sequence).  This is the value the backward's
 *                                              pass 1 calls sig.  With activate == 0, values[k, c] = tmp.
 *                               sigma[k]     = features[r, K - 1], the stored bits.
 *                             A sample whose row is outside [0, M) gets values = 0, sigma = 0 and no gradient
 *                             (svoxt_gather_rows' rule); so does, for its values, a sample whose ray is outside [0, Q).
 *                             A lane per (sample, channel) plus one per sample for sigma; RGBA rows of K = 4 n floats in a
 *                             16-byte aligned table: a lane per (sample, four columns), 16-byte loads.  T = 0: a no-op.
 *                             Checked: options not NULL, the format, K >= 1, T, M, Q in [0, 2^31); with a basis basis_dim
 *                             in [1, 25] and min_comp / max_comp inside [0, basis_dim); T * (C + 1) and M * K below 2^38;
 *                             with T > 0: row, sigma, values (C > 0) not NULL, features not NULL when M > 0, with a basis
 *                             ray and basis not NULL; alignment (4 bytes).
 *
 *   svoxt_shade_samples_bwd   grad float32 [M, K], the gradient with respect to features for grad_values [T, C] and
 *                             grad_sigma [T] (either may be NULL: zeros, nothing is read for it).  Every element of grad
 *                             is written.
 *                               colour column (c, i), i in the component range: the sum over the row's samples of
 *                                              (grad_values[k, c] * d[k, c]) * basis[ray[k], i].  With activate != 0 and a
 *                                              basis, d = (float)((double)sig * (1.0 - (double)sig)); for RGBA, d = sig *
 *                                              (1.f - sig) and there is no basis factor; sig = values[k, c], the forward's
 *                                              own output.  With activate == 0 the factor is grad_values[k, c] alone.
 *                               sigma column   the sum of grad_sigma[k].
 *                               every other column, and rows no sample names: exactly 0.f.
 *                             The sum order is svoxt_reduce_rows' rule: samples in ascending index over the plan (row_ptr,
 *                             perm, long_rows, long_chunk_ptr, chunk_long, n_long, n_chunks: svoxt_row_plan_build /
 *                             svoxt_row_plan_long of the same row array and M), chunks of SVOXT_ROW_CHUNK = 256 from 0.f,
 *                             the partials in chunk order.  A lane per (row, column) over all K columns, the value of
 *                             sample k at column j formed on the fly.  workspace: svoxt_shade_samples_bwd_workspace_bytes(
 *                             n_chunks, K) device bytes (-1: n_chunks negative or from 2^31, K < 1, n_chunks * K from 2^38;
 *                             0 for n_chunks = 0), 4-byte aligned.  M = 0: a no-op; T = 0: zeros everywhere.
 *                             Checked: as the forward; n_long and n_chunks as svoxt_row_plan_long; with M > 0: grad,
 *                             row_ptr not NULL; with T > 0 perm and what the given gradients make it read (values, ray,
 *                             basis) not NULL; with n_long > 0 long_rows, long_chunk_ptr, chunk_long not NULL; alignment
 *                             (4 bytes); with n_long > 0 the workspace not NULL and at least the query's size.
 *
 * The gradient in the view direction: the view-dependent half of a gradient in the rays, beside
 * svoxt_sample_geometry_bwd.  Two gathers, float32 without contraction, no float atomic, no [T, K] array, no workspace:
 * every result is bit-identical from run to run.  Entry points added under ABI v22.
 *
 *   svoxt_view_basis_bwd      grad_vdirs float32 [Q, 3] for grad_basis float32 [Q, basis_dim] and basis, the forward's own
 *                             [Q, basis_dim] (read for SG only; may be NULL otherwise).  A lane per ray, every ray written.
 *                             With (x, y, z) = rays.vdirs[q] AS GIVEN -- the forward does not normalise the direction, so
 *                             the derivative is not projected on the sphere -- and g_i = grad_basis[q, i]: three
 *                             accumulators gx, gy, gz from 0.f, and for i ascending
 *                                 gx += g_i * X_i;  gy += g_i * Y_i;  gz += g_i * Z_i        (product rounded, then the add)
 *                             with (X_i, Y_i, Z_i) the analytic derivative of the expression svoxt_view_basis evaluates
 *                             for component i; a partial written `.` below is identically zero and is NOT added.  THIS
 *                             SEQUENCE IS THE DEFINITION.  SH, with the constants C1, C2[5], C3[7], C4[9] of the forward
 *                             and xx = x * x, yy, zz, xy = x * y, yz = y * z, xz = x * z, every product and difference
 *                             one float32 operation in the order written (left to right):
 *                                 i     X_i                          Y_i                           Z_i
 *                                 0     .                            .                             .
 *                                 1     .                            -C1                           .
 *                                 2     .                            .                             C1
 *                                 3     -C1                          .                             .
 *                                 4     C2[0] * y                    C2[0] * x                     .
 *                                 5     .                            C2[1] * z                     C2[1] * y
 *                                 6     C2[2] * (-2 * x)             C2[2] * (-2 * y)              C2[2] * (4 * z)
 *                                 7     C2[3] * z                    .                             C2[3] * x
 *                                 8     C2[4] * (2 * x)              C2[4] * (-2 * y)              .
 *                                 9     C3[0] * (6 * xy)             C3[0] * a                     .
 *                                 10    C3[1] * yz                   C3[1] * xz                    C3[1] * xy
 *                                 11    C3[2] * (-2 * xy)            C3[2] * (4 * zz - xx - 3 * yy)   C3[2] * (8 * yz)
 *                                 12    C3[3] * (-6 * xz)            C3[3] * (-6 * yz)             C3[3] * (6 * zz - 3 * xx - 3 * yy)
 *                                 13    C3[4] * (4 * zz - 3 * xx - yy)   C3[4] * (-2 * xy)         C3[4] * (8 * xz)
 *                                 14    C3[5] * (2 * xz)             C3[5] * (-2 * yz)             C3[5] * (xx - yy)
 *                                 15    C3[6] * a                    C3[6] * (-6 * xy)             .
 *                                 16    C4[0] * (y * p)              C4[0] * (x * m)               .
 *                                 17    C4[1] * ((6 * xy) * z)       C4[1] * (z * a)               C4[1] * (y * p)
 *                                 18    C4[2] * (y * s1)             C4[2] * (x * s1)              C4[2] * ((14 * xy) * z)
 *                                 19    .                            C4[3] * (z * s3)              C4[3] * (y * t3)
 *                                 20    .                            .                             C4[4] * (z * (140 * zz - 60))
 *                                 21    C4[5] * (z * s3)             .                             C4[5] * (x * t3)
 *                                 22    C4[6] * ((2 * x) * s1)       C4[6] * ((-2 * y) * s1)       C4[6] * ((xx - yy) * (14 * z))
 *                                 23    C4[7] * (z * a)              C4[7] * ((-6 * xy) * z)       C4[7] * (x * m)
 *                                 24    C4[8] * (x * (4 * xx - 12 * yy))   C4[8] * (y * (4 * yy - 12 * xx))   .
 *                             a = 3 * xx - 3 * yy, p = 3 * xx - yy, m = xx - 3 * yy, s1 = 7 * zz - 1, s3 = 7 * zz - 3,
 *                             t3 = 21 * zz - 3.  (Component 6 is formed through double in the forward; its derivative is
 *                             the float32 line above.)  Only the components basis_dim holds (1 / 4 / 9 / 16 / 25).
 *                             SG, lobe i = extra_data[i, :]:    s = basis[q, i] * lobe[0];  (X, Y, Z) = s * lobe[1 .. 3]
 *                                 -- the forward's own output, no exponential is computed.
 *                             ASG:  S, dot_x, dot_y and E = expf(-lobe[0] * dot_x * dot_x - lobe[1] * dot_y * dot_y) by the
 *                                 forward's sequence (E is recomputed, never out_i / S: S may be 0);  SE = S * E;
 *                                 cx = (-2 * lobe[0]) * dot_x;  cy = (-2 * lobe[1]) * dot_y;  for the axis a = 0, 1, 2:
 *                                 (lobe[8 + a] * E + SE * (cx * lobe[2 + a] + cy * lobe[5 + a])) / (float)basis_dim
 *                             The gradient in the lobe parameters (extra_data) is not formed.  Checked: as
 *                             svoxt_view_basis; rays.c2w NULL (camera mode has no viewdirs tensor to receive a gradient);
 *                             tree.xform NULL; grad_basis, grad_vdirs (SG: basis) not NULL; alignment (4 bytes).  RGBA and
 *                             Q = 0: a no-op.
 *
 *   svoxt_shade_samples_bwd_basis   grad_basis float32 [Q, basis_dim], the gradient with respect to svoxt_shade_samples_fwd's
 *                             basis for grad_values [T, C] over the lists (offsets int64 [Q + 1], row, ray).  Every
 *                             element is written.  THIS SEQUENCE IS THE DEFINITION, for every ray q and component i in
 *                             [min_comp, max_comp]:
 *                                 acc = 0.f
 *                                 for k = max(offsets[q], 0) .. min(offsets[q + 1], T) - 1, in list order:
 *                                     if ray[k] == q and 0 <= row[k] < M:
 *                                         for c = 0 .. C - 1:
 *                                             acc += (grad_values[k, c] * d[k, c]) * features[row[k], c * basis_dim + i]
 *                                 grad_basis[q, i] = acc
 *                             d[k, c] = (float)((double)sig * (1.0 - (double)sig)), sig = values[k, c], the forward's own
 *                             output: the factor of svoxt_shade_samples_bwd, so the two gradients of one forward agree
 *                             term for term.  With activate == 0 the bracket is grad_values[k, c] alone and values is not
 *                             read.  For i outside [min_comp, max_comp] grad_basis[q, i] = 0.f and nothing is read; a ray
 *                             without samples gets zeros.  A sample standing in ray q's segment whose ray[k] is another
 *                             ray contributes nothing (svoxt_ray_samples_emit never writes one).  basis_dim lanes a ray walk
 *                             its segment together; a workgroup holds whole rays.  grad_values NULL, C = 0 or T = 0: zeros,
 *                             nothing is read.  RGBA and Q = 0: a no-op.  Checked: as svoxt_shade_samples_fwd; offsets
 *                             (8-byte aligned), grad_basis not NULL; with a gradient to read: row, ray, values (activate
 *                             != 0), features (M > 0) not NULL; alignment (4 bytes).
 * No allocation, no synchronisation. */
int svoxt_view_basis(const svoxt_tree* tree, const svoxt_rays* rays, const svoxt_options* opt, float* basis, void* stream);
int svoxt_view_basis_bwd(const svoxt_tree* tree, const svoxt_rays* rays, const svoxt_options* opt, const float* basis,
                         const float* grad_basis, float* grad_vdirs, void* stream);
int svoxt_shade_samples_bwd_basis(const float* features, int64_t M, int32_t K, const svoxt_options* opt, const int64_t* offsets,
                                  const int32_t* row, const int32_t* ray, int64_t T, int64_t Q, int32_t activate,
                                  const float* values, const float* grad_values, float* grad_basis, void* stream);
int svoxt_shade_samples_fwd(const float* features, int64_t M, int32_t K, const svoxt_options* opt, const int32_t* row,
                            const int32_t* ray, int64_t T, const float* basis, int64_t Q, int32_t activate, float* values,
                            float* sigma, void* stream);
int64_t svoxt_shade_samples_bwd_workspace_bytes(int64_t n_chunks, int32_t K);
int svoxt_shade_samples_bwd(const svoxt_options* opt, int64_t M, int32_t K, const int32_t* ray, int64_t T, const float* basis,
                            int64_t Q, int32_t activate, const float* values, const float* grad_values,
                            const float* grad_sigma, const int32_t* row_ptr, const int32_t* perm, const int32_t* long_rows,
                            const int32_t* long_chunk_ptr, const int32_t* chunk_long, int64_t n_long, int64_t n_chunks,
                            float* grad, void* workspace, int64_t workspace_bytes, void* stream);

/* ---- shade_samples with per-row rotations of the view direction (svoxt_viewrot.hip) ----
 * What the render kernels do with tree.xform, for the per-sample interface: the basis of sample k is evaluated at its ray's
 * view direction rotated by its FEATURE ROW's matrix, and the colour is differentiable in the table, in the matrices and in
 * the directions.  The reference has no gradient in the matrices.  Explicit pointers, no svoxt_tree: features float32
 * [M, K]; rotations float32 [M, rot_dim, rot_dim], rot_dim 3 or 4, of which the upper-left 3 x 3 is read; viewdirs float32
 * [Q, 3]; extra float32 [extra_rows, extra_cols], the lobes of SG / ASG (tree.extra_data; not read for SH).  Float32
 * without contraction, no float atomic, no [T, basis_dim] and no [T, K] array: every result is bit-identical from run to
 * run.  Entry points added under ABI v22.  A format with a basis only: RGBA is refused (svoxt_shade_samples_* serve it).
 *
 * THE DEFINITION.  For sample k with row r = row[k] and ray q = ray[k], d = rot_dim, m = rotations + r * d * d and
 * (v0, v1, v2) = viewdirs[q] as given -- nothing is normalised:
 *     u0 = m[0] * v0 + m[1] * v1 + m[2] * v2;   u1 = m[d] * v0 + m[d + 1] * v1 + m[d + 2] * v2;
 *     u2 = m[2 d] * v0 + m[2 d + 1] * v1 + m[2 d + 2] * v2                       (left to right, every operation rounded)
 *     B[0 .. basis_dim) = the basis values svoxt_view_basis forms at the direction (u0, u1, u2)
 *     tmp = 0.f;  for i = min_comp .. max_comp: tmp += B[i] * features[r, c * basis_dim + i]
 *     values[k, c] = activate ? (float)(1.0 / (1.0 + (double)expf(-tmp))) : tmp;      sigma[k] = features[r, K - 1]
 * A sample whose row is outside [0, M) gets values = 0 and sigma = 0, one whose ray is outside [0, Q) values = 0; neither
 * takes part in any gradient.
 *
 *   svoxt_shade_rot_fwd       values float32 [T, C], sigma float32 [T].  A lane per (sample, channel) and one per sample for
 *                             sigma; the SH sizes at compile time, the basis in registers; SG / ASG one lobe at a time.
 *                             T = 0: a no-op.
 *   svoxt_shade_rot_bwd       grad float32 [M, K] for grad_values [T, C] / grad_sigma [T] (either may be NULL: zeros).
 *                             Every element is written.  Colour column (c, i), i in the component range: the sum over the
 *                             row's samples of (grad_values[k, c] * d[k, c]) * B_i(k) -- activate == 0: grad_values[k, c] *
 *                             B_i(k) --, d[k, c] = (float)((double)sig * (1.0 - (double)sig)), sig = values[k, c], B_i(k)
 *                             recomputed from m and v by the forward's sequence; the sigma column: the sum of
 *                             grad_sigma[k]; every other column 0.f.  The order is svoxt_reduce_rows' over the plan of
 *                             `row` and M (samples ascending, chunks of SVOXT_ROW_CHUNK from 0.f, the partials in chunk
 *                             order).  A lane per (row, column) loads the row's matrix once.  workspace:
 *                             svoxt_shade_samples_bwd_workspace_bytes(n_chunks, K).  M = 0: a no-op.
 *   svoxt_shade_rot_bwd_dir   gu float32 [T, 3], the gradient in (u0, u1, u2) of every sample -- the one per-sample array
 *                             the next two entry points read, 12 bytes a sample.  With t[k, c] = grad_values[k, c] *
 *                             d[k, c] (activate == 0: grad_values[k, c]):
 *                                 gB_i = 0.f;  for c = 0 .. C - 1: gB_i += t[k, c] * features[r, c * basis_dim + i]
 *                                                                            (0.f for i outside [min_comp, max_comp])
 *                                 gu[k, :] = svoxt_view_basis_bwd's sequence at the direction (u0, u1, u2) with grad_basis =
 *                                            gB: the same table of partials, the same ascending order; SG multiplies by
 *                                            B_i(k) recomputed by the forward's sequence where that operator reads its
 *                                            saved output; ASG as there.
 *                             Zeros for a sample outside its ranges and for grad_values NULL (or C = 0).  A lane per
 *                             sample, C = 3 with t in registers.  T = 0: a no-op.
 *   svoxt_shade_rot_bwd_rotations   grad_rotations float32 [M, rot_dim, rot_dim], every element written, zeros outside the
 *                             3 x 3 block: grad[r, a, b] = the sum over the row's samples, in svoxt_reduce_rows' order over
 *                             the same plan, of gu[k, a] * viewdirs[ray[k], b] (0.f for a ray outside [0, Q)).  A lane per
 *                             (row, a, b).  workspace: svoxt_shade_samples_bwd_workspace_bytes(n_chunks, rot_dim *
 *                             rot_dim).  M = 0: a no-op.
 *   svoxt_shade_rot_bwd_viewdirs    grad_vdirs float32 [Q, 3], every ray written, zeros without samples.  A lane per ray,
 *                             three accumulators from 0.f, over k = max(offsets[q], 0) .. min(offsets[q + 1], T) - 1 in
 *                             list order; a sample with ray[k] != q or a row outside [0, M) is passed over; else
 *                                 for a = 0, 1, 2:  for b = 0, 1, 2:  acc[b] += m[a * d + b] * gu[k, a]
 *                             Q = 0: a no-op.
 * Checked, before any launch: options not NULL, a format with a basis, basis_dim in [1, 25] (SH: 1, 4, 9, 16 or 25),
 * min_comp / max_comp inside [0, basis_dim), SG / ASG: extra not NULL with at least basis_dim rows and 4 / 11 columns;
 * rot_dim 3 or 4; K >= 1; T, M, Q in [0, 2^31); T * (C + 1) and M * K below 2^38; n_long / n_chunks as svoxt_row_plan_long;
 * what is read or written not NULL; alignment (4 bytes; offsets 8); no output overlapping an input (or the other output);
 * with n_long > 0 the workspace not NULL and at least the query's size.  No allocation, no synchronisation. */
int svoxt_shade_rot_fwd(const float* features, int64_t M, int32_t K, const svoxt_options* opt, const float* extra,
                        int32_t extra_rows, int32_t extra_cols, const float* rotations, int32_t rot_dim, const float* viewdirs,
                        int64_t Q, const int32_t* row, const int32_t* ray, int64_t T, int32_t activate, float* values,
                        float* sigma, void* stream);
int svoxt_shade_rot_bwd(const svoxt_options* opt, int64_t M, int32_t K, const float* extra, int32_t extra_rows,
                        int32_t extra_cols, const float* rotations, int32_t rot_dim, const float* viewdirs, int64_t Q,
                        const int32_t* row, const int32_t* ray, int64_t T, int32_t activate, const float* values,
                        const float* grad_values, const float* grad_sigma, const int32_t* row_ptr, const int32_t* perm,
                        const int32_t* long_rows, const int32_t* long_chunk_ptr, const int32_t* chunk_long, int64_t n_long,
                        int64_t n_chunks, float* grad, void* workspace, int64_t workspace_bytes, void* stream);
int svoxt_shade_rot_bwd_dir(const float* features, int64_t M, int32_t K, const svoxt_options* opt, const float* extra,
                            int32_t extra_rows, int32_t extra_cols, const float* rotations, int32_t rot_dim,
                            const float* viewdirs, int64_t Q, const int32_t* row, const int32_t* ray, int64_t T,
                            int32_t activate, const float* values, const float* grad_values, float* gu, void* stream);
int svoxt_shade_rot_bwd_rotations(const float* gu, const float* viewdirs, int64_t Q, const int32_t* ray, int64_t T, int64_t M,
                                  int32_t rot_dim, const int32_t* row_ptr, const int32_t* perm, const int32_t* long_rows,
                                  const int32_t* long_chunk_ptr, const int32_t* chunk_long, int64_t n_long, int64_t n_chunks,
                                  float* grad_rotations, void* workspace, int64_t workspace_bytes, void* stream);
int svoxt_shade_rot_bwd_viewdirs(const float* gu, const float* rotations, int32_t rot_dim, int64_t M, const int64_t* offsets,
                                 const int32_t* row, const int32_t* ray, int64_t T, int64_t Q, float* grad_vdirs, void* stream);

/* ---- interp: a trilinear lookup over the leaves around a point (svoxt_interp.hip; not in the reference)
 * A lookup that is continuous in position where svoxt_query_fwd is piecewise constant, with the gradients with respect
 * to the table and to the point.  Gather only, a fixed float32 order, no float atomic: every result is bit-identical
 * from run to run.  Entry points added under ABI v22.  Every float operation below is a separate float32 operation
 * without contraction; everything else is integer arithmetic.  Finite points are the contract.
 *
 * THE STENCIL of a point p: eight feature rows and eight weights.
 *   1. Locate     Transform, clamp and descend exactly as svoxt_query_fwd does (one shared function).  This gives the
 *                 leaf slot, its depth d, cube_sz = N^(d + 1), the leaf-local coordinates l in [0, 1)^3 and the leaf's
 *                 integer cell coordinate c in [0, N^(d + 1))^3: the digits of the descent, svoxt_leaf_neighbors'
 *                 definition of a cell.
 *   2. Per axis a u = l_a - 0.5f;  s_a = (u < 0) ? -1 : +1;  f_a = |u|;  g_a = 1.0f - f_a.
 *   3. Corners    Corner j = 4 b_x + 2 b_y + b_z with b in {0, 1}^3.  Its cell is t = c + (b_x s_x, b_y s_y, b_z s_z) at
 *                 the leaf's own level.  Its weight is w_j = (m_x * m_y) * m_z with m_a = b_a ? f_a : g_a.  Corner 0 is
 *                 the leaf itself.
 *   4. The row of corner j, t inside the cube: ONE integer descent from node 0 by the base-N digits of t for the levels
 *                 0 .. d.  If it ends at a leaf of depth <= d, that leaf's data word is taken.  If the cell is still a
 *                 node after level d, finer leaves cover it: the descent continues with the digits of the cell's centre
 *                 -- for an even N digit N / 2 once and then digit 0, for an odd N digit (N - 1) / 2 at every level --
 *                 until a leaf (at most 64 levels further).  By construction this is the leaf svoxt_query_fwd reports at
 *                 the centre X_j of cell t_j:  interp(p) = sum over j of w_j * query(X_j).
 *   5. Corners without a row: t outside the cube, a data word outside [0, M), a descent that leaves the tables.
 *                 fill = SVOXT_INTERP_FILL_SELF: the corner takes the query leaf's own row (clamp to the edge: the hard
 *                 silhouette of the piecewise-constant field stays).  SVOXT_INTERP_FILL_ZERO: it takes row -1.
 *   6. An empty query leaf (its data word outside [0, M)): all eight rows are -1.  The weights are written as in 3.
 *   Depth limits are svoxt_leaf_neighbors': where N^(d + 1) >= 2^31 the cell coordinate is not formed and the corners
 *   1 .. 7 count as corners without a row.
 * THE VALUE      out[q, jc] = sum over j = 0 .. 7 of w_j * table[rows[q, j], cols[jc]]:  acc = 0;  acc = acc + w_j * v_j in
 *                ascending j; corners with a row outside [0, M) are skipped.
 * THE TABLE GRADIENT  G[r, c] = the sum over the entries e = 8 q + j with rows[e] = r of w_e * g[e >> 3, c], in
 *                svoxt_reduce_rows' order over the row plan of `rows` viewed as int32 [8 Q]: ascending e, chunks of
 *                SVOXT_ROW_CHUNK from 0.f, the partials in chunk order.  Every element of [M, K] is written.
 * THE POINT GRADIENT  D_j = sum over the selected columns jc, ascending, from 0.f, of g[q, jc] * v_{j, jc} (0 for a skipped
 *                corner).  Per axis a: S_a = sum over j, ascending, from 0.f, of sigma_{j,a} * (m_a' * m_a'') * D_j, where
 *                sigma_{j,a} = b_a ? +1 : -1 (a change of sign, exact) and a' < a'' are the other two axes.
 *                grad_points[q, a] = ((S_a * s_a) * cube_sz) * scaling[a], and 0 on an axis whose coordinate the clamp
 *                changed.  The exact derivative of the value as defined, inside a leaf.
 * KNOWN PROPERTIES, stated and not hidden: the field is continuous inside leaves and across faces between leaves of
 * equal depth; it is NOT continuous across a change of level.  No parity claim: the reference has no such operator.
 *
 *   svoxt_interp_stencil      rows int32 [Q, 8], weights float32 [Q, 8] for points float32 [Q, 3].  A lane per point, an
 *                             N = 2 and a generic-N instance; 16-byte stores where rows and weights are 16-byte aligned.
 *                             tree.features is not read (tree.M decides which data words name a row).  Q = 0: a no-op.
 *                             Checked: the tree (as svoxt_query_fwd), N <= 16; Q in [0, 2^28) (8 Q < 2^31), M in
 *                             [0, 2^31); fill among the constants; with Q > 0 points, rows, weights not NULL, 4-byte aligned.
 *   svoxt_interp_rows_fwd     out float32 [Q, C] (C = n_cols, or K without cols) from table float32 [M, K].  The lanes of a
 *                             point move its rows together; 16 bytes a lane where all columns are taken, K is a multiple
 *                             of 4 and table and out are 16-byte aligned, else 4 ("Alignment" above): the same bits.
 *                             Checked: Q, M; K >= 1; cols / n_cols NULL / 0 or n_cols in [1, K]; Q * C and M * K below
 *                             2^38; with Q > 0: rows, weights, out not NULL, table not NULL when M > 0, alignment (4 bytes).
 *   svoxt_interp_rows_bwd     grad float32 [M, K] from grad_out float32 [Q, C] over the plan (svoxt_row_plan_build /
 *                             svoxt_row_plan_long of rows as int32 [8 Q] and M).  workspace:
 *                             svoxt_interp_rows_bwd_workspace_bytes(n_chunks, C) device bytes (-1 / 0 as
 *                             svoxt_reduce_rows_workspace_bytes), 4-byte aligned.  M = 0: a no-op.
 *                             Checked: Q, M; K, cols / n_cols; C = n_cols (or K); Q * C and M * K below 2^38; n_long and
 *                             n_chunks as svoxt_row_plan_long with T = 8 Q; with M > 0: grad, row_ptr not NULL; with Q > 0
 *                             grad_out, weights, perm not NULL; with n_long > 0 the long-row arrays not NULL; alignment
 *                             (4 bytes); with n_long > 0 the workspace not NULL and at least the query's size.
 *   svoxt_interp_points_bwd   grad_points float32 [Q, 3]: locates again for s, f and cube_sz; eight lanes per point, lane j
 *                             forms D_j (16-byte loads where all columns are taken, K is a multiple of 4 and table and
 *                             grad_out are 16-byte aligned, else 4: the same order, the same bits).
 *                             Checked: the tree, N <= 16; Q, M; K, cols / n_cols; the 2^38 bounds; with Q > 0 points, rows,
 *                             grad_out, grad_points not NULL, table not NULL when M > 0; alignment (4 bytes).
 * No allocation, no synchronisation. */
#define SVOXT_INTERP_FILL_SELF 0
#define SVOXT_INTERP_FILL_ZERO 1
int svoxt_interp_stencil(const svoxt_tree* tree, const float* points, int64_t Q, int32_t fill, int32_t* rows, float* weights,
                         void* stream);
int svoxt_interp_rows_fwd(const float* table, int64_t M, int32_t K, const int32_t* rows, const float* weights, int64_t Q,
                          const int32_t* cols, int32_t n_cols, float* out, void* stream);
int64_t svoxt_interp_rows_bwd_workspace_bytes(int64_t n_chunks, int32_t C);
int svoxt_interp_rows_bwd(const float* grad_out, const float* weights, int64_t Q, int32_t C, const int32_t* row_ptr,
                          const int32_t* perm, int64_t M, const int32_t* long_rows, const int32_t* long_chunk_ptr,
                          const int32_t* chunk_long, int64_t n_long, int64_t n_chunks, const int32_t* cols, int32_t n_cols,
                          int32_t K, float* grad, void* workspace, int64_t workspace_bytes, void* stream);
int svoxt_interp_points_bwd(const svoxt_tree* tree, const float* points, int64_t Q, const int32_t* rows, const float* table,
                            int64_t M, int32_t K, const int32_t* cols, int32_t n_cols, const float* grad_out,
                            float* grad_points, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SVOXT_H_ */
