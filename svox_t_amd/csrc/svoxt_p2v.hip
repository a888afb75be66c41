// svoxt_p2v.hip -- voxelize: the Gaussian splat of per-point density into a dense [n, n, n, 1] grid and its
// gradient (the reference's p2v / p2v_backward, svox_t/csrc/p2v_kernel.cu:104-285).
//
// The reference runs a thread per point and adds every (point, voxel) term with a float atomic, so 64 lanes hit 64
// unrelated addresses and the sums change from run to run.  Here the forward is a gather, with no float atomics and
// a fixed order of addition per voxel:
//   1. key: each point is binned by the 4x4x4 tile of its window's lower corner (the window is the reference's
//      floor / ceil box, clamped); non-finite points and points farther than conv_radius + one voxel from the volume
//      go to a last bin that nobody reads.  Per-bin counts (integer atomics, one per distinct key in a wavefront) are
//      scanned into the bins' starts.
//   2. a stable LSD radix sort of (key, point index), passes of <= 8 bits: per-workgroup histogram, exclusive scan
//      (svoxt_order.hip's two kernels), a scatter that ranks equal digits within a wavefront with ballots.  Inside a
//      bin the points stay in ascending index order.
//   3. records: the sorted points' xyz, last feature column and packed window, contiguous.
//   4. work items: a tile's candidates are the bins of its apron (the tiles whose points can reach it), in fixed
//      (x, y, z) order -- for each (x, y) a run of consecutive z bins, i.e. one contiguous range of records.  Each
//      tile's candidate list is cut into chunks of kP2VChunk: one wavefront per chunk, one voxel per lane.  The chunk
//      count depends only on the bin counts, so the split is the same in every run.
//   5. gather: chunk 0 stores its 64 sums into the volume, chunk j > 0 into a partial slot; 6. a second launch adds
//      the partials of multi-chunk tiles in chunk order.  No workgroup waits for another.
// Every (point, voxel) pair is decided by the reference's float expressions in the reference's order (this unit is
// built with -ffp-contract=off), so the pair set is exactly the reference's; sums run over bins in fixed order and,
// inside a bin, over ascending point index, so the volume is bit-identical from run to run.
//
// The backward is the reference's per-point loop (x -> y -> z, the same expressions) with the sums in registers: one
// thread per point, each output element written once; the points are walked in the forward's sorted order when the
// caller passes it, so neighbouring lanes read neighbouring grad_output.

#include <math.h>
#include <hip/hip_runtime.h>

#include "svoxt_host.h"
#include "svoxt_sort.h"
#include "svoxt_workspace.h"

namespace svoxt {

constexpr int kP2VTile = 4;                 // tiles of 4x4x4 voxels: a wavefront each
constexpr int kP2VChunk = 1024;             // candidates per work item
constexpr int kP2VBlock = 256;
constexpr size_t kGatherBlocksMax = (size_t)1 << 18;             // beyond 1 M work items the gather's waves stride

struct P2VGeom {
    float cx, cy, cz;                       // volume_corner
    float vx, vy, vz;                       // voxel size: volume_size / (n - 1), as the reference computes it
    float kx0, ky0, kz0, kx1, ky1, kz1;     // points outside [k0, k1] have no pair: the volume box grown by cr + a voxel
    float cr, den;                          // conv_radius, 2 * kernel_radius * kernel_radius
    int n, T;                               // voxels and tiles per axis
    int ax, ay, az;                         // apron: the bins of tiles t - a .. t per axis can reach tile t
    uint32_t nt;                            // T^3; key nt = dropped
};

// the reference's window on one axis (p2v_kernel.cu:122-127): floor / ceil of ((p -/+ cr) - corner) / voxel_size,
// clamped to [0, n - 1] (here in float, which equals the reference's clamp of the converted value for every finite
// point it keeps)
__device__ __forceinline__ void p2v_axis(float p, float c, float vs, float cr, int n, int& lo, int& hi) {
    const float top = (float)(n - 1);
    lo = (int)fminf(fmaxf(floorf(((p - cr) - c) / vs), 0.f), top);
    hi = (int)fminf(fmaxf(ceilf(((p + cr) - c) / vs), 0.f), top);
}

__device__ __forceinline__ bool p2v_finite(float x, float y, float z) {
    return isfinite(x) && isfinite(y) && isfinite(z);
}

// the records of bins (bx, by, tz - az .. tz): consecutive keys, so one range [s, e)
__device__ __forceinline__ void p2v_range(const uint32_t* __restrict__ bin_start, const P2VGeom& g, int bx, int by, int tz,
                                          uint32_t& s, uint32_t& e) {
    const uint32_t row = ((uint32_t)bx * g.T + (uint32_t)by) * g.T;
    s = bin_start[row + (uint32_t)max(0, tz - g.az)];
    e = bin_start[row + (uint32_t)tz + 1];
}

// 1. keys and per-bin counts.  A wavefront sends one atomic per distinct key (clustered clouds put thousands of
// points in one bin).
__global__ void __launch_bounds__(kP2VBlock)
p2v_key_kernel(const float* __restrict__ pts, uint32_t P, P2VGeom g, uint32_t* __restrict__ keys, uint32_t* __restrict__ counts) {
    const uint32_t i = blockIdx.x * kP2VBlock + threadIdx.x;
    uint32_t key = g.nt;
    if (i < P) {
        const float x = pts[3 * (size_t)i], y = pts[3 * (size_t)i + 1], z = pts[3 * (size_t)i + 2];
        if (p2v_finite(x, y, z) && x >= g.kx0 && x <= g.kx1 && y >= g.ky0 && y <= g.ky1 && z >= g.kz0 && z <= g.kz1) {
            int lx, hx, ly, hy, lz, hz;
            p2v_axis(x, g.cx, g.vx, g.cr, g.n, lx, hx);
            p2v_axis(y, g.cy, g.vy, g.cr, g.n, ly, hy);
            p2v_axis(z, g.cz, g.vz, g.cr, g.n, lz, hz);
            key = ((uint32_t)(lx / kP2VTile) * g.T + (uint32_t)(ly / kP2VTile)) * g.T + (uint32_t)(lz / kP2VTile);
        }
        keys[i] = key;
    }
    bool todo = i < P;
    while (__ballot(todo)) {
        const int first = __ffsll((unsigned long long)__ballot(todo)) - 1;
        const uint32_t lead = (uint32_t)__shfl((int)key, first, 64);
        const bool mine = todo && key == lead;
        const unsigned long long same = __ballot(mine);
        if ((int)(threadIdx.x & 63) == first) atomicAdd(&counts[lead], (uint32_t)__popcll(same));
        todo = todo && !mine;
    }
}

// 2. the sort's passes: svoxt_sort.h (shared with svoxt_quant.hip)

// 3. the records the gather reads, in sorted order: xyz + last feature column, and the window packed 10 bits an axis
__global__ void __launch_bounds__(kP2VBlock)
p2v_records_kernel(const float* __restrict__ pts, const float* __restrict__ feats, int F, const uint32_t* __restrict__ order,
                   const uint32_t* __restrict__ bin_start, P2VGeom g, float4* __restrict__ rec, uint2* __restrict__ win) {
    const uint32_t k = blockIdx.x * kP2VBlock + threadIdx.x;
    if (k >= bin_start[g.nt]) return;                        // the dropped points (last bin) are never read
    const size_t i = order[k];
    const float x = pts[3 * i], y = pts[3 * i + 1], z = pts[3 * i + 2];
    int lx, hx, ly, hy, lz, hz;
    p2v_axis(x, g.cx, g.vx, g.cr, g.n, lx, hx);
    p2v_axis(y, g.cy, g.vy, g.cr, g.n, ly, hy);
    p2v_axis(z, g.cz, g.vz, g.cr, g.n, lz, hz);
    rec[k] = make_float4(x, y, z, feats[i * F + (F - 1)]);
    win[k] = make_uint2((uint32_t)lx | (uint32_t)ly << 10 | (uint32_t)lz << 20, (uint32_t)hx | (uint32_t)hy << 10 | (uint32_t)hz << 20);
}

// 4a. work items per tile: max(1, ceil(candidates / kP2VChunk)); n_items[nt] = 0 closes the scan
__global__ void __launch_bounds__(kP2VBlock)
p2v_tile_items_kernel(const uint32_t* __restrict__ bin_start, P2VGeom g, uint32_t* __restrict__ n_items) {
    const uint32_t t = blockIdx.x * kP2VBlock + threadIdx.x;
    if (t > g.nt) return;
    if (t == g.nt) { n_items[t] = 0; return; }
    const int tx = (int)(t / ((uint32_t)g.T * g.T)), ty = (int)(t / g.T % g.T), tz = (int)(t % g.T);
    uint32_t c = 0;
    for (int bx = max(0, tx - g.ax); bx <= tx; ++bx)
        for (int by = max(0, ty - g.ay); by <= ty; ++by) {
            uint32_t s, e;
            p2v_range(bin_start, g, bx, by, tz, s, e);
            c += e - s;
        }
    n_items[t] = c == 0 ? 1u : (c + kP2VChunk - 1) / kP2VChunk;
}

// 4b. the tile of every work item
__global__ void __launch_bounds__(kP2VBlock)
p2v_item_list_kernel(const uint32_t* __restrict__ item_start, uint32_t nt, uint32_t* __restrict__ item_tile) {
    const uint32_t t = blockIdx.x * kP2VBlock + threadIdx.x;
    if (t >= nt) return;
    for (uint32_t it = item_start[t]; it < item_start[t + 1]; ++it) item_tile[it] = t;
}

// 5. one wavefront per work item, one voxel per lane; the waves of the grid stride over the items (the grid is sized
// for the items there are at most, capped: no host read).  Chunk j > 0 of tile t stores into partial slot
// item_start[t] - t + j - 1 (the tiles before t have that many chunks past their first).
__global__ void __launch_bounds__(kP2VBlock)
p2v_gather_kernel(const float4* __restrict__ rec, const uint2* __restrict__ win, const uint32_t* __restrict__ bin_start,
                  const uint32_t* __restrict__ item_start, const uint32_t* __restrict__ item_tile, P2VGeom g,
                  float* __restrict__ voxels, float* __restrict__ partial) {
    const uint32_t lane = threadIdx.x & 63, total = item_start[g.nt];
    const uint64_t stride = (uint64_t)gridDim.x * (kP2VBlock / 64);
    for (uint64_t it = (uint64_t)blockIdx.x * (kP2VBlock / 64) + (threadIdx.x >> 6); it < total; it += stride) {
        const uint32_t item = (uint32_t)it;
        const uint32_t t = item_tile[item], j = item - item_start[t];
        const int tx = (int)(t / ((uint32_t)g.T * g.T)), ty = (int)(t / g.T % g.T), tz = (int)(t % g.T);
        const int vx = tx * kP2VTile + (int)(lane >> 4), vy = ty * kP2VTile + (int)((lane >> 2) & 3), vz = tz * kP2VTile + (int)(lane & 3);
        // p_voxel = i * voxel_size + corner (p2v_kernel.cu:133)
        const float px = (float)vx * g.vx + g.cx, py = (float)vy * g.vy + g.cy, pz = (float)vz * g.vz + g.cz;
        const uint32_t tlx = (uint32_t)tx * kP2VTile, tly = (uint32_t)ty * kP2VTile, tlz = (uint32_t)tz * kP2VTile;
        const uint32_t c0 = j * kP2VChunk, c1 = c0 + kP2VChunk;
        uint32_t pos = 0;                                        // candidates in the ranges before the current one
        float acc = 0.f;
        for (int bx = max(0, tx - g.ax); bx <= tx; ++bx)
            for (int by = max(0, ty - g.ay); by <= ty; ++by) {
                uint32_t s, e;
                p2v_range(bin_start, g, bx, by, tz, s, e);
                const uint32_t len = e - s;
                if (pos < c1 && pos + len > c0) {
                    const uint32_t a = s + (c0 > pos ? c0 - pos : 0u), b = s + min(len, c1 - pos);
                    // 64 candidates at a time: one coalesced load (a lane a record), then each in turn from its lane
                    for (uint32_t base = a; base < b; base += 64) {
                        const uint32_t m = min(64u, b - base), k = base + min(lane, m - 1);
                        const uint2 wl = win[k];
                        const float4 pl = rec[k];
                        for (uint32_t q = 0; q < m; ++q) {
                            const uint32_t w0 = (uint32_t)__builtin_amdgcn_readlane((int)wl.x, (int)q);
                            const uint32_t w1 = (uint32_t)__builtin_amdgcn_readlane((int)wl.y, (int)q);
                            const uint32_t lx = w0 & 1023u, ly = (w0 >> 10) & 1023u, lz = w0 >> 20;
                            const uint32_t hx = w1 & 1023u, hy = (w1 >> 10) & 1023u, hz = w1 >> 20;
                            if (hx < tlx || lx > tlx + 3 || hy < tly || ly > tly + 3 || hz < tlz || lz > tlz + 3) continue;  // misses the tile
                            if ((uint32_t)vx >= lx && (uint32_t)vx <= hx && (uint32_t)vy >= ly && (uint32_t)vy <= hy &&
                                (uint32_t)vz >= lz && (uint32_t)vz <= hz) {
                                const float dx = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(pl.x), (int)q)) - px;
                                const float dy = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(pl.y), (int)q)) - py;
                                const float dz = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(pl.z), (int)q)) - pz;
                                const float sigma = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(pl.w), (int)q));
                                const float r = sqrtf(dx * dx + dy * dy + dz * dz);
                                if (r <= g.cr) acc = acc + expf(-r * r / g.den) * sigma;
                            }
                        }
                    }
                }
                pos += len;
            }
        if (j == 0) {
            if (vx < g.n && vy < g.n && vz < g.n) voxels[((size_t)vx * g.n + vy) * g.n + vz] = acc;
        } else {
            partial[((size_t)(item_start[t] - t) + j - 1) * 64 + lane] = acc;
        }
    }
}

// 6. tiles of more than one chunk: chunk 0's sums (in the volume) + the partials, in chunk order
__global__ void __launch_bounds__(kP2VBlock)
p2v_reduce_kernel(const uint32_t* __restrict__ item_start, P2VGeom g, float* __restrict__ voxels, const float* __restrict__ partial) {
    const uint32_t t = blockIdx.x * (kP2VBlock / 64) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (t >= g.nt) return;
    const uint32_t first = item_start[t], nch = item_start[t + 1] - first;
    if (nch <= 1) return;
    const int tx = (int)(t / ((uint32_t)g.T * g.T)), ty = (int)(t / g.T % g.T), tz = (int)(t % g.T);
    const int vx = tx * kP2VTile + (int)(lane >> 4), vy = ty * kP2VTile + (int)((lane >> 2) & 3), vz = tz * kP2VTile + (int)(lane & 3);
    if (vx >= g.n || vy >= g.n || vz >= g.n) return;
    const size_t at = ((size_t)vx * g.n + vy) * g.n + vz;
    const float* q = partial + (size_t)(first - t) * 64 + lane;
    float acc = voxels[at];
    for (uint32_t c = 1; c < nch; ++c) acc = acc + q[(size_t)(c - 1) * 64];
    voxels[at] = acc;
}

// backward: the reference's loop per point (p2v_kernel.cu:170-214) with the sums in registers
__global__ void __launch_bounds__(kP2VBlock)
p2v_backward_kernel(const float* __restrict__ gout, const float* __restrict__ pts, const float* __restrict__ feats, int F, uint32_t P,
                    const int32_t* __restrict__ order, P2VGeom g, float kk, float* __restrict__ points_grad,
                    float* __restrict__ features_grad) {
    const uint32_t k = blockIdx.x * kP2VBlock + threadIdx.x;
    if (k >= P) return;
    const size_t i = order != nullptr ? (size_t)(uint32_t)order[k] : k;
    const float x = pts[3 * i], y = pts[3 * i + 1], z = pts[3 * i + 2];
    float gx = 0.f, gy = 0.f, gz = 0.f, gf = 0.f;
    if (p2v_finite(x, y, z)) {                               // non-finite points: zero gradient
        int lx, hx, ly, hy, lz, hz;
        p2v_axis(x, g.cx, g.vx, g.cr, g.n, lx, hx);
        p2v_axis(y, g.cy, g.vy, g.cr, g.n, ly, hy);
        p2v_axis(z, g.cz, g.vz, g.cr, g.n, lz, hz);
        const float f = feats[i * F + (F - 1)];
        for (int a = lx; a <= hx; ++a)
            for (int b = ly; b <= hy; ++b)
                for (int c = lz; c <= hz; ++c) {
                    const float dx = x - ((float)a * g.vx + g.cx), dy = y - ((float)b * g.vy + g.cy), dz = z - ((float)c * g.vz + g.cz);
                    const float r = sqrtf(dx * dx + dy * dy + dz * dz);
                    if (r <= g.cr) {
                        const float w = expf(-r * r / g.den);
                        const float go = gout[((size_t)a * g.n + b) * g.n + c];
                        gf = gf + go * w;
                        const float wg = go * f;
                        gx = gx + -wg * dx * w / kk;
                        gy = gy + -wg * dy * w / kk;
                        gz = gz + -wg * dz * w / kk;
                    }
                }
    }
    if (points_grad != nullptr) {
        points_grad[3 * i] = gx;
        points_grad[3 * i + 1] = gy;
        points_grad[3 * i + 2] = gz;
    }
    if (features_grad != nullptr) {
        for (int c = 0; c < F - 1; ++c) features_grad[i * F + c] = 0.f;
        features_grad[i * F + (F - 1)] = gf;
    }
}

// Argument checks shared by the three entry points; fills the geometry.  Nothing here touches HIP.
static int p2v_setup(int64_t P, int32_t F, const float* corner, const float* size, int32_t n, float kr, float cr,
                     P2VGeom& g, const char* fn) {
    if (n < 2 || n > 1024) return set_error(SVOXT_ERR_INVALID, "%s: n_voxels must be in [2, 1024]", fn);
    if (!(kr > 0.f)) return set_error(SVOXT_ERR_INVALID, "%s: kernel_radius must be > 0", fn);
    if (!(cr >= 0.f) || !isfinite(cr)) return set_error(SVOXT_ERR_INVALID, "%s: conv_radius must be finite and >= 0", fn);
    if (P < 0 || P > 0x7fffffff) return set_error(SVOXT_ERR_INVALID, "%s: the number of points must be in [0, 2^31)", fn);
    if (F < 1) return set_error(SVOXT_ERR_INVALID, "%s: point_features needs at least one column", fn);
    if (corner == nullptr || size == nullptr) return set_error(SVOXT_ERR_INVALID, "%s: volume_corner / volume_size is NULL", fn);
    for (int a = 0; a < 3; ++a) {
        if (!isfinite(corner[a])) return set_error(SVOXT_ERR_INVALID, "%s: volume_corner must be finite", fn);
        if (!(size[a] > 0.f) || !isfinite(size[a])) return set_error(SVOXT_ERR_INVALID, "%s: volume_size must be finite and > 0", fn);
    }
    const float vs[3] = {size[0] / (float)(n - 1), size[1] / (float)(n - 1), size[2] / (float)(n - 1)};
    g.cx = corner[0]; g.cy = corner[1]; g.cz = corner[2];
    g.vx = vs[0]; g.vy = vs[1]; g.vz = vs[2];
    g.cr = cr;
    g.den = 2 * kr * kr;                                     // (2 * kernel_radius) * kernel_radius in float, as written there
    g.n = n;
    g.T = (n + kP2VTile - 1) / kP2VTile;
    g.nt = (uint32_t)g.T * g.T * g.T;
    int apron[3];
    float lo[3], hi[3];
    for (int a = 0; a < 3; ++a) {
        // kept points lie within cr + a voxel of the box, so their windows are at most W voxels wide: 2 cr / vs, plus 2
        // for floor / ceil, plus a bound on the rounding of the window's float expressions (an ulp of the largest
        // magnitude involved, in voxels, taken 16x over)
        const double c = corner[a], v = vs[a], R = (double)cr / v;
        const double mag = (2.0 * fabs(c) + (double)size[a] + 2.0 * cr + v) / v + n + 2.0 * R + 4.0;
        const double W = floor(2.0 * R + 2.0 * mag * ldexp(1.0, -21)) + 2.0;
        apron[a] = (int)fmin(ceil(W / kP2VTile), (double)(g.T - 1));
        lo[a] = (float)(c - cr - v);
        hi[a] = (float)(c + (double)size[a] + cr + v);
    }
    g.ax = apron[0]; g.ay = apron[1]; g.az = apron[2];
    g.kx0 = lo[0]; g.ky0 = lo[1]; g.kz0 = lo[2];
    g.kx1 = hi[0]; g.ky1 = hi[1]; g.kz1 = hi[2];
    return SVOXT_OK;
}

struct P2VSpace {
    uint32_t nblocks, bits;                  // sort workgroups, key bits
    size_t max_items, max_slots, scan_words;
    uint32_t *keys[2], *vals[2], *counts, *bins, *items, *item_tile, *sort_counts, *sort_starts, *chunks;
    float4* rec;
    uint2* win;
    float* partial;
    size_t bytes;
};

static bool p2v_carve(void* workspace, int64_t P, const P2VGeom& g, P2VSpace& p) {
    // candidates over all tiles: every point at most once per tile of its apron.  One tile has at most P of them (< 2^31);
    // what has to fit 32 bits is the number of work items, tiles + candidates / kP2VChunk (checked below)
    const double cand = (double)P * (g.ax + 1) * (g.ay + 1) * (g.az + 1);
    p.nblocks = sort_blocks((uint64_t)P);
    p.bits = 0;
    while ((g.nt >> p.bits) != 0) ++p.bits;                  // the dropped key nt included
    p.max_slots = (size_t)(cand / kP2VChunk) + 1;
    p.max_items = (size_t)g.nt + p.max_slots;
    if ((double)g.nt + cand / kP2VChunk + 2.0 >= 4294967296.0) return false;
    const size_t tiles = (size_t)g.nt + 1, sortw = (size_t)256 * p.nblocks;
    p.scan_words = exclusive_scan_chunks(tiles > sortw ? tiles : sortw);
    const size_t n = (size_t)P;
    Carver w(workspace);
    for (int b = 0; b < 2; ++b) { p.keys[b] = w.take<uint32_t>(n); p.vals[b] = w.take<uint32_t>(n); }
    p.rec = w.take<float4>(n);
    p.win = w.take<uint2>(n);
    p.counts = w.take<uint32_t>(tiles);
    p.bins = w.take<uint32_t>(tiles);
    p.items = w.take<uint32_t>(tiles);
    p.item_tile = w.take<uint32_t>(p.max_items);
    p.sort_counts = w.take<uint32_t>(sortw);
    p.sort_starts = w.take<uint32_t>(sortw);
    p.chunks = w.take<uint32_t>(p.scan_words);
    p.partial = w.take<float>(64 * p.max_slots);
    p.bytes = w.bytes();
    return true;
}

}  // namespace svoxt

using namespace svoxt;

extern "C" {

int64_t svoxt_p2v_workspace_bytes(int64_t P, int32_t n_voxels, const float* volume_corner, const float* volume_size,
                                  float conv_radius) {
    P2VGeom g;
    P2VSpace p;
    // the same setup and plan as the forward's (the apron's rounding bound depends on the corner)
    if (p2v_setup(P, 1, volume_corner, volume_size, n_voxels, 1.f, conv_radius, g, "svoxt_p2v_workspace_bytes") != SVOXT_OK) return -1;
    if (!p2v_carve(nullptr, P, g, p)) return -1;
    return (int64_t)p.bytes;
}

int svoxt_p2v_fwd(const float* points, const float* point_features, int64_t P, int32_t F, const float* volume_corner,
                  const float* volume_size, int32_t n_voxels, float kernel_radius, float conv_radius, float* voxels,
                  int32_t* order, void* workspace, int64_t workspace_bytes, void* stream) {
    const char* fn = "svoxt_p2v_fwd";
    P2VGeom g;
    int rc;
    if ((rc = p2v_setup(P, F, volume_corner, volume_size, n_voxels, kernel_radius, conv_radius, g, fn))) return rc;
    P2VSpace p;
    if (!p2v_carve(workspace, P, g, p)) return set_error(SVOXT_ERR_UNSUPPORTED, "%s: conv_radius spans too many tiles for this many points", fn);
    if (P > 0 && workspace_bytes < (int64_t)p.bytes) return set_error(SVOXT_ERR_INVALID, "%s: workspace too small", fn);
    if (P > 0 && workspace == nullptr) return set_error(SVOXT_ERR_INVALID, "%s: workspace is NULL", fn);
    if (voxels == nullptr) return set_error(SVOXT_ERR_INVALID, "%s: voxels is NULL", fn);
    if (P > 0 && (points == nullptr || point_features == nullptr)) return set_error(SVOXT_ERR_INVALID, "%s: points / point_features is NULL", fn);
    hipStream_t st = (hipStream_t)stream;
    if (P == 0) {
        const size_t nvox = (size_t)n_voxels * n_voxels * n_voxels;
        const hipError_t e = hipMemsetAsync(voxels, 0, sizeof(float) * nvox, st);
        return e == hipSuccess ? SVOXT_OK : set_error(SVOXT_ERR_HIP, "%s: hipMemsetAsync: %s", fn, hipGetErrorString(e));
    }
    const uint32_t n = (uint32_t)P, tiles = g.nt + 1;
    const unsigned nb = (n + kP2VBlock - 1) / kP2VBlock, waves = kP2VBlock / 64;

    hipError_t e = hipMemsetAsync(p.counts, 0, sizeof(uint32_t) * tiles, st);
    if (e != hipSuccess) return set_error(SVOXT_ERR_HIP, "%s: hipMemsetAsync: %s", fn, hipGetErrorString(e));
    hipLaunchKernelGGL(p2v_key_kernel, dim3(nb), dim3(kP2VBlock), 0, st, points, n, g, p.keys[0], p.counts);
    if ((rc = check_launch(fn)) || (rc = exclusive_scan(p.counts, tiles, p.chunks, p.bins, st, fn))) return rc;
    // stable LSD radix sort of (key, point index)
    int cur = 0;
    for (uint32_t shift = 0; shift < p.bits; shift += 8) {
        const int bits = (int)(p.bits - shift < 8 ? p.bits - shift : 8);
        if ((rc = sort_pass(p.keys[cur], shift == 0 ? nullptr : p.vals[cur], n, (int)shift, bits, p.sort_counts, p.sort_starts, p.chunks,
                            p.keys[cur ^ 1], p.vals[cur ^ 1], st, fn))) return rc;
        cur ^= 1;
    }
    const uint32_t* sorted = p.vals[cur];
    hipLaunchKernelGGL(p2v_records_kernel, dim3(nb), dim3(kP2VBlock), 0, st, points, point_features, (int)F, sorted, p.bins, g, p.rec, p.win);
    hipLaunchKernelGGL(p2v_tile_items_kernel, dim3((tiles + kP2VBlock - 1) / kP2VBlock), dim3(kP2VBlock), 0, st, p.bins, g, p.counts);
    if ((rc = check_launch(fn)) || (rc = exclusive_scan(p.counts, tiles, p.chunks, p.items, st, fn))) return rc;
    hipLaunchKernelGGL(p2v_item_list_kernel, dim3((g.nt + kP2VBlock - 1) / kP2VBlock), dim3(kP2VBlock), 0, st, p.items, g.nt, p.item_tile);
    const size_t gather_blocks = (p.max_items + waves - 1) / waves;
    hipLaunchKernelGGL(p2v_gather_kernel, dim3((unsigned)(gather_blocks < kGatherBlocksMax ? gather_blocks : kGatherBlocksMax)), dim3(kP2VBlock), 0, st, p.rec, p.win, p.bins,
                       p.items, p.item_tile, g, voxels, p.partial);
    hipLaunchKernelGGL(p2v_reduce_kernel, dim3((g.nt + waves - 1) / waves), dim3(kP2VBlock), 0, st, p.items, g, voxels, p.partial);
    if ((rc = check_launch(fn))) return rc;
    if (order != nullptr) {
        e = hipMemcpyAsync(order, sorted, sizeof(uint32_t) * n, hipMemcpyDeviceToDevice, st);
        if (e != hipSuccess) return set_error(SVOXT_ERR_HIP, "%s: hipMemcpyAsync: %s", fn, hipGetErrorString(e));
    }
    return SVOXT_OK;
}

int svoxt_p2v_bwd(const float* grad_output, const float* points, const float* point_features, int64_t P, int32_t F,
                  const float* volume_corner, const float* volume_size, int32_t n_voxels, float kernel_radius, float conv_radius,
                  const int32_t* order, float* points_grad, float* point_features_grad, void* stream) {
    const char* fn = "svoxt_p2v_bwd";
    P2VGeom g;
    int rc;
    if ((rc = p2v_setup(P, F, volume_corner, volume_size, n_voxels, kernel_radius, conv_radius, g, fn))) return rc;
    if (P > 0 && (grad_output == nullptr || points == nullptr || point_features == nullptr))
        return set_error(SVOXT_ERR_INVALID, "%s: grad_output / points / point_features is NULL", fn);
    if (P == 0 || (points_grad == nullptr && point_features_grad == nullptr)) return SVOXT_OK;
    const float kk = kernel_radius * kernel_radius;
    hipLaunchKernelGGL(p2v_backward_kernel, dim3((unsigned)((P + kP2VBlock - 1) / kP2VBlock)), dim3(kP2VBlock), 0, (hipStream_t)stream,
                       grad_output, points, point_features, (int)F, (uint32_t)P, order, g, kk, points_grad, point_features_grad);
    return check_launch(fn);
}

}  // extern "C"
