/*
 * bev_submap_pn_vox.h — a voxel grid and 2-D normals over the UNION of a map's moved PointNormal rows, between the
 * concatenation of bev_submap_coarse.h and its ICP (bev_submap_coarse_voxel_registration_device_resident,
 * bev_submap_pn_cloud_device_resident):
 *   V = bev_voxel_grid_xyz(positions of concat(g), pn_leaf), N = bev_normals_2d(V, radius, viewpoint),
 *   target(g)[i] = the PointNormal record of V[i] and N[i].
 * The moved normals and curvatures of concat(g) are not used: the normals are RECOMPUTED over the union.  Per launch group of
 * the plan (bev_submap_reg_plan.h with point_normal and union_voxel), the sort as bev_submap_vox_plan.h schedules it:
 *   k_submap_pn_move     per map         : submap_pn_concat, k_submap_pn_target's first two steps (bev_submap_coarse.h):
 *                                          concat(g) into the moved rows, its count
 *   k_submap_pn_keys     per map         : rf_voxel_bounds and rf_voxel_keys over the moved rows' positions: the union's
 *                                          bounds, divisions and overflow test, the keys voxel index << 32 | concatenation
 *                                          index, padded with ~0 to the map's own power of two
 *   k_submap_vox_tile, k_submap_vox_global (bev_submap_vox.h) as they are: they see key arrays and headers only
 *   k_submap_pn_finish   per map         : rf_voxel_starts (the voxel's index recorded), then rf_voxel_centroids (key order
 *                                          is concatenation order) into the position array; the overflow branch copies the
 *                                          moved rows to the target instead
 *   k_submap_pn_normals  per (part, map) : one lane per thinned point: Normal2d (bev_regfront.h), k_rf_normals' arithmetic,
 *                                          over a window of the union's grid in THREE dimensions, the candidates staged in
 *                                          LDS, see below; 12-float rows
 *   k_submap_pn_grid     per map         : reg_grid_build<kIcpCells> over the target's positions
 *   k_submap_out (bev_submap_vox.h)      : the cloud call: a map's rows and count into the caller's arrays
 * then k_submap_coarse_icp and k_icp_best as they are, the SubmapCoarseWork pointing at the thinned rows.
 * A map's point count is known on the device only: the grids are the plan's (the group's largest capacity), and a workgroup
 * beyond its map's count returns at once.  No float sum depends on an atomic or on which workgroup ran first: a centroid and
 * a point's neighbour sums are one lane's loops.  Every workgroup has 256 threads.
 * Part of the device code of libbev_mi355x.so; included by bev_kernels.hip only (one translation unit).
 */
#ifndef BEV_SUBMAP_PN_VOX_H
#define BEV_SUBMAP_PN_VOX_H

#include "bev_submap_reg_plan.h"

namespace bevk {

static_assert(bevsubreg::kCoarseUnionRowBytes == 48 + 16 + 48 + 4 + 4 + 16,
              "the thinned row and its searchable copy, the moved row, a voxel start, a voxel index, a position");

/* Map map0 + blockIdx.x of the plan: submap_pn_concat (bev_submap_coarse.h) into p.moved; the header's n and n_out (with
 * pn_leaf == 0 the moved rows are the cloud call's target) */
__global__ __launch_bounds__(kIcpThreads) void k_submap_pn_move(const bevsubreg::Map *maps, uint32_t map0,
                                                                const bevsubreg::Entry *entries, const float *pn, size_t stride,
                                                                const uint32_t *counts, uint32_t *ent_start, SubmapPnVoxWork p)
{
    __shared__ uint32_t wave_sum[kRegWaves];
    __shared__ uint32_t s_base;
    const bevsubreg::Map mp = maps[map0 + blockIdx.x];
    const uint32_t n = submap_pn_concat(mp, entries, pn, stride, counts, ent_start, p.moved + mp.pt0 * 12, wave_sum, s_base);
    if (threadIdx.x == 0) {
        SubvoxHdr h{};
        h.n = h.n_out = n;
        p.v.vh[blockIdx.x] = h;
    }
}

/* map map0 + blockIdx.x: k_submap_vox_keys' steps (bev_submap_vox.h; a body of its own, see there) on the moved rows'
 * positions; the union grid's divisions into the header */
__global__ __launch_bounds__(kIcpThreads) void k_submap_pn_keys(const bevsubreg::Map *maps, uint32_t map0, SubmapPnVoxWork p,
                                                                float pn_leaf)
{
    __shared__ float red[7 * kRegWaves];
    __shared__ int s_par[8]; /* overflow, nfin, minb xyz, div xyz */
    const int g = (int)blockIdx.x, t = (int)threadIdx.x;
    const uint32_t n = p.v.vh[g].n;
    const IcpRows fetch{p.moved + maps[map0 + g].pt0 * 12};
    const float inv = 1.0f / pn_leaf;
    rf_voxel_bounds(n, fetch, inv, red, s_par);
    const uint32_t nf = (uint32_t)s_par[1];
    const bool sort = nf != 0 && !s_par[0];
    const uint32_t np2 = sort ? rf_pow2(n) : 0u;
    if (t == 0) {
        SubvoxHdr &h = p.v.vh[g];
        h.np2 = np2;
        h.nf = nf;
        h.overflow = nf != 0 && s_par[0];
        for (int d = 0; d < 3; ++d) h.div[d] = sort ? (uint32_t)s_par[5 + d] : 0u;
    }
    if (sort) rf_voxel_keys(n, np2, fetch, inv, s_par, p.v.keys + p.v.key0[map0 + g]);
}

/* map map0 + blockIdx.x: the thinned positions p.vpos + pt0 and their voxel indices p.vidx + pt0, the count in vh[g].n_out;
 * the overflow branch: the moved rows, as they are, into the target rows */
__global__ __launch_bounds__(kIcpThreads) void k_submap_pn_finish(const bevsubreg::Map *maps, uint32_t map0, SubmapPnVoxWork p,
                                                                  float *target)
{
    __shared__ uint32_t wave_cnt[kRegWaves];
    const int g = (int)blockIdx.x, tid = (int)threadIdx.x;
    const uint64_t pt0 = maps[map0 + g].pt0;
    const SubvoxHdr h = p.v.vh[g];
    const float4 *moved = reinterpret_cast<const float4 *>(p.moved + pt0 * 12);
    uint32_t n_out = 0;
    if (h.nf == 0) {
        /* no finite position: an empty target */
    } else if (h.overflow) { /* PCL: "leaf size is too small": the target is the concatenation, moved normals included */
        float4 *to = reinterpret_cast<float4 *>(target + pt0 * 12);
        for (uint32_t i = tid; i < 3u * h.n; i += kRegThreads) to[i] = moved[i];
        n_out = h.n;
    } else {
        const uint64_t *buf = p.v.keys + p.v.key0[map0 + g];
        uint32_t *vstart = p.v.vstart + pt0 + g; /* (cap + 1 words per map) */
        uint32_t *vidx = p.vidx + pt0;
        float4 *vpos = p.vpos + pt0;
        n_out = rf_voxel_starts(buf, h.nf, wave_cnt, vstart, [=](uint32_t v, uint32_t i) { vidx[v] = (uint32_t)(buf[i] >> 32); });
        __syncthreads();
        rf_voxel_centroids(buf, vstart, n_out, [moved](uint32_t i) { return moved[(size_t)i * 3]; }, vpos);
    }
    if (tid == 0) p.v.vh[g].n_out = n_out;
}

/* The 256 thinned points from blockIdx.x * 256 on of map map0 + blockIdx.y, one lane each, the candidates staged in LDS.
 * A voxel's index is i + j * div_x + k * div_x * div_y and the thinned points are sorted by it; a centroid lies in its voxel
 * (or rounds just outside: the + 2 of win), so every point within the radius of a query in row j_q of layer k_q lies in the
 * layers k_q +- win and there in the rows j_q +- win: per layer one contiguous range of indices, found by two binary searches.
 * The workgroup's queries are 256 CONSECUTIVE indices, from (k0, j0) to (k1, j1), so the union of their windows is, in every
 * layer k0 - win .. k1 + win: the rows j0 - win .. j1 + win where k0 == k1; the rows 0 .. j1 + win and j0 - win .. div_y - 1
 * (two ranges, or one where they meet) where the queries cross from one layer into the next; every row where they span more.
 * The workgroup walks that union, layers ascending and ranges ascending inside, in chunks of kSubpnStage positions, every lane
 * testing every staged candidate: a superset of its own neighbours in ascending index, which is all the contract's sums need,
 * and all lanes read one LDS address at a time.  Where div_x * div_y * div_z does not fit 32 bits an index is known only modulo
 * 2^32: one range, every point.  Surplus workgroups (the grid is sized by the capacity) and maps in the overflow branch
 * return at once.  Measured against one lane walking its own window in global memory: DESIGN.md §6q. */
constexpr uint32_t kSubpnStage = 1024;
__global__ __launch_bounds__(kIcpThreads) void k_submap_pn_normals(const bevsubreg::Map *maps, uint32_t map0, SubmapPnVoxWork p,
                                                                   float r2, uint32_t win, float vpx, float vpy, float *target)
{
    __shared__ float4 s_pts[kSubpnStage];
    const uint32_t g = blockIdx.y;
    const SubvoxHdr h = p.v.vh[g];
    const uint32_t v0 = blockIdx.x * kRegThreads, nv = h.n_out;
    if (h.overflow || v0 >= nv) return; /* (workgroup-uniform) */
    const uint32_t tid = threadIdx.x, v = v0 + tid;
    const bool active = v < nv;
    const uint64_t pt0 = maps[map0 + g].pt0;
    const float4 *pts = p.vpos + pt0;
    const uint32_t *vidx = p.vidx + pt0;
    Normal2d nrm;
    nrm.q = active ? pts[v] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    nrm.r2 = r2;
    /* the union of the queries' windows: layers kl .. kh, in each the row ranges [rl[i], rh[i]], i < nr (all workgroup-uniform) */
    const uint64_t layer = (uint64_t)h.div[0] * h.div[1];
    const bool windowed = layer * (uint64_t)h.div[2] < (1ull << 32) && layer < (1ull << 32);
    uint32_t kl = 0, kh = 0, nr = 1, rl[2] = {0u, 0u}, rh[2] = {0u, 0u};
    if (windowed) {
        const uint32_t first = vidx[v0], last = vidx[min(v0 + kRegThreads, nv) - 1u], top = h.div[1] - 1u;
        const uint32_t k0 = first / (uint32_t)layer, j0 = (first - k0 * (uint32_t)layer) / h.div[0];
        const uint32_t k1 = last / (uint32_t)layer, j1 = (last - k1 * (uint32_t)layer) / h.div[0];
        const uint32_t below = j0 > win ? j0 - win : 0u, above = (uint32_t)min((uint64_t)j1 + win, (uint64_t)top);
        kl = k0 > win ? k0 - win : 0u;
        kh = (uint32_t)min((uint64_t)k1 + win, (uint64_t)h.div[2] - 1u);
        rl[0] = 0u, rh[0] = top;
        if (k0 == k1) {
            rl[0] = below, rh[0] = above;
        } else if (k1 == k0 + 1u && above + 1u < below) {
            rh[0] = above;
            rl[1] = below, rh[1] = top;
            nr = 2;
        }
    }
    for (int pass = 0; pass < 2; ++pass) {
        if (pass == 1) {
            if (nrm.cnt >= 3) nrm.mean();
            if (!__syncthreads_or(active && nrm.cnt >= 3)) break;
        }
        const bool mine = active && (pass == 0 || nrm.cnt >= 3);
        for (uint32_t k = kl; k <= kh; ++k)
            for (uint32_t r = 0; r < nr; ++r) {
                const uint32_t lo = windowed ? rf_lower_bound(vidx, nv, k * layer + (uint64_t)rl[r] * h.div[0]) : 0u;
                const uint32_t hi = windowed ? rf_lower_bound(vidx, nv, k * layer + ((uint64_t)rh[r] + 1u) * h.div[0]) : nv;
                for (uint32_t base = lo; base < hi; base += kSubpnStage) {
                    const uint32_t n = min(kSubpnStage, hi - base);
                    __syncthreads(); /* (the chunk before is read) */
                    for (uint32_t t = tid; t < n; t += kRegThreads) s_pts[t] = pts[base + t];
                    __syncthreads();
                    if (mine) {
                        if (pass == 0)
                            for (uint32_t t = 0; t < n; ++t) nrm.first(base + t, s_pts[t]);
                        else
                            for (uint32_t t = 0; t < n; ++t) nrm.second(s_pts[t]);
                    }
                }
            }
    }
    if (active) nrm.write<true>(pts, vpx, vpy, reinterpret_cast<float4 *>(target + (pt0 + v) * 12));
}

/* map map0 + blockIdx.x: the search grid of the target's n_out positions, as k_submap_pn_target's step 3 */
__global__ __launch_bounds__(kIcpThreads) void k_submap_pn_grid(const bevsubreg::Map *maps, uint32_t map0, const SubvoxHdr *vh,
                                                                SubmapCoarseWork t)
{
    const uint64_t pt0 = maps[map0 + blockIdx.x].pt0;
    reg_grid_build<kIcpCells>(vh[blockIdx.x].n_out, IcpRows{t.rows + pt0 * 12}, t.hdr + blockIdx.x,
                              t.cell_off + (size_t)blockIdx.x * (kIcpCells + 1), t.sorted + pt0);
}

void launch_submap_pn_move(const void *maps, uint32_t map0, int n_maps, const void *entries, const float *pn, size_t stride,
                           const uint32_t *counts, uint32_t *ent_start, const SubmapPnVoxWork &p, hipStream_t st)
{
    if (n_maps > 0)
        hipLaunchKernelGGL(k_submap_pn_move, dim3(n_maps), dim3(kIcpThreads), 0, st, static_cast<const bevsubreg::Map *>(maps), map0,
                           static_cast<const bevsubreg::Entry *>(entries), pn, stride, counts, ent_start, p);
}

void launch_submap_pn_keys(const void *maps, uint32_t map0, int n_maps, const SubmapPnVoxWork &p, float pn_leaf, hipStream_t st)
{
    if (n_maps > 0)
        hipLaunchKernelGGL(k_submap_pn_keys, dim3(n_maps), dim3(kIcpThreads), 0, st, static_cast<const bevsubreg::Map *>(maps), map0,
                           p, pn_leaf);
}

void launch_submap_pn_finish(const void *maps, uint32_t map0, int n_maps, const SubmapPnVoxWork &p, float *target, hipStream_t st)
{
    if (n_maps > 0)
        hipLaunchKernelGGL(k_submap_pn_finish, dim3(n_maps), dim3(kIcpThreads), 0, st, static_cast<const bevsubreg::Map *>(maps),
                           map0, p, target);
}

void launch_submap_pn_normals(const void *maps, uint32_t map0, int n_maps, uint32_t parts, const SubmapPnVoxWork &p, float radius,
                              float pn_leaf, const float vp[2], float *target, hipStream_t st)
{
    if (n_maps <= 0 || parts == 0) return;
    const float r2 = (float)((double)radius * (double)radius);
    /* rows and layers of the window: the radius in voxels, +2 for a centroid that rounds just outside its voxel */
    const double rows = std::ceil((double)radius / (double)pn_leaf) + 2.0;
    const uint32_t win = rows < 4294967295.0 ? (uint32_t)rows : 0xffffffffu;
    hipLaunchKernelGGL(k_submap_pn_normals, dim3(parts, (uint32_t)n_maps), dim3(kIcpThreads), 0, st,
                       static_cast<const bevsubreg::Map *>(maps), map0, p, r2, win, vp[0], vp[1], target);
}

void launch_submap_pn_grid(const void *maps, uint32_t map0, int n_maps, const SubvoxHdr *vh, const SubmapCoarseWork &t,
                           hipStream_t st)
{
    if (n_maps > 0)
        hipLaunchKernelGGL(k_submap_pn_grid, dim3(n_maps), dim3(kIcpThreads), 0, st, static_cast<const bevsubreg::Map *>(maps), map0,
                           vh, t);
}

} /* namespace bevk */

#endif /* BEV_SUBMAP_PN_VOX_H */
