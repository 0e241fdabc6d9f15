/*
 * bev_icp.h — coarse point-to-plane ICP (included by bev_kernels.hip): pcl::IterativeClosestPointWithNormals<PointNormal,
 * PointNormal> as performCoarseIcp runs it (BatchTopPartRegistration.cpp:192-221), on the registration front end's
 * PointNormal clouds.  The contract every line follows (and tests/icp/icp_oracle.c restates) is DESIGN.md §6c.
 *
 *   k_icp_grid   per target frame : bounds of the searchable points (finite x, y, z), a uniform 2-D grid of at most
 *                                   kIcpGridMax^2 square cells, a counting sort of the points by cell (x, y, z, index)
 *   k_icp        per problem      : the whole ICP loop of one (match, guess) in one workgroup — correspondences, the
 *                                   27 LLS sums and the MSE in the pinned order, the 6 x 6 solve, the increment,
 *                                   convergence — then getFitnessScore
 *   k_icp_best   per match        : guess 0 iff fitness0 < fitness1
 *
 * The grid build, the search (icp_nn), the ordered pass and the loop around the estimator are bev_reg_common.h's.
 * Exact 1-NN: ring search on the grid, lowest index on equal distance.  The grid is only an accelerator: the order of the
 * points inside a cell (an atomic) changes nothing, and a ring is skipped only when a lower bound on the xy distance of
 * every point in it, taken with a wide margin for rounding, exceeds the best distance (or D^2).  No float or double sum
 * depends on an atomic: every sum runs over 64-point chunks as a fixed tree (wave shuffles), the chunks in ascending
 * order in one lane.  Point i of the source is transformed, read and written by thread i % 256 only.
 */
#pragma once

namespace bevk {

__global__ __launch_bounds__(kIcpThreads) void k_icp_grid(const float *pn, size_t stride, const uint32_t *counts,
                                                          const uint32_t *slot_frame, IcpWork w)
{
    const uint32_t frame = slot_frame[blockIdx.x];
    reg_grid_build<kIcpCells>(min(counts[frame], (uint32_t)stride), IcpRows{pn + (size_t)frame * stride * 12},
                              w.hdr + blockIdx.x, w.cell_off + (size_t)blockIdx.x * (kIcpCells + 1),
                              w.sorted + (size_t)blockIdx.x * stride);
}

struct IcpShared {
    RegSums<0, 28> sums;
    RegLoop loop;
    IcpGridHdr hdr;
    uint32_t off[kIcpCells + 1];
};

/* thread 0: the 6 x 6 solve, the increment (constructTransformationMatrix), then the shared tail */
__device__ void icp_step(IcpShared &sh, const bev_icp_params_t &prm, double &prev)
{
    double M[6][6], v[6], x[6];
    bool ok[6];
    {
        int k = 0;
        for (int a = 0; a < 6; ++a)
            for (int b = a; b < 6; ++b) M[a][b] = M[b][a] = sh.sums.totd[k++];
        for (int a = 0; a < 6; ++a) v[a] = sh.sums.totd[21 + a];
    }
    for (int k = 0; k < 6; ++k) {
        ok[k] = M[k][k] > 0.0;
        if (!ok[k]) continue;
        for (int i = k + 1; i < 6; ++i) {
            const double f = M[i][k] / M[k][k];
            for (int j = k + 1; j < 6; ++j) M[i][j] -= f * M[k][j];
            v[i] -= f * v[k];
        }
    }
    for (int k = 5; k >= 0; --k) {
        if (!ok[k]) {
            x[k] = 0.0;
            continue;
        }
        double s = v[k];
        for (int j = k + 1; j < 6; ++j) s -= M[k][j] * x[j];
        x[k] = s / M[k][k];
    }
    /* constructTransformationMatrix(alpha, beta, gamma, tx, ty, tz) */
    const double sa = bevx::fd_sin(x[0]), ca = bevx::fd_cos(x[0]), sb = bevx::fd_sin(x[1]), cb = bevx::fd_cos(x[1]);
    const double sg = bevx::fd_sin(x[2]), cg = bevx::fd_cos(x[2]);
    float *I = sh.loop.inc;
    I[0] = (float)(cg * cb);
    I[1] = (float)(-sg * ca + cg * sb * sa);
    I[2] = (float)(sg * sa + cg * sb * ca);
    I[3] = (float)x[3];
    I[4] = (float)(sg * cb);
    I[5] = (float)(cg * ca + sg * sb * sa);
    I[6] = (float)(-cg * sa + sg * sb * ca);
    I[7] = (float)x[4];
    I[8] = (float)(-sb);
    I[9] = (float)(cb * sa);
    I[10] = (float)(cb * ca);
    I[11] = (float)x[5];
    I[12] = 0.0f;
    I[13] = 0.0f;
    I[14] = 0.0f;
    I[15] = 1.0f;
    reg_converge(sh.loop, prm, sh.sums.totd[27], sh.sums.cnt, prev);
}

__global__ __launch_bounds__(kIcpThreads) void k_icp(const float *pn, size_t stride, const uint32_t *counts,
                                                     const IcpProblem *probs, IcpWork w, bev_icp_params_t prm,
                                                     bev_icp_result_t *results)
{
    __shared__ IcpShared sh;
    const int tid = threadIdx.x;
    const IcpProblem pb = probs[blockIdx.x];
    const uint32_t n_src = min(counts[pb.src_frame], (uint32_t)stride);
    const float *src = pn + (size_t)pb.src_frame * stride * 12;
    const float *tgt = pn + (size_t)pb.tgt_frame * stride * 12;
    const float4 *tpts = w.sorted + (size_t)pb.tgt_slot * stride;
    float4 *cur = w.cur + (size_t)(blockIdx.x % kIcpProblemsPerLaunch) * stride;
    if (tid == 0) sh.hdr = w.hdr[pb.tgt_slot];
    __syncthreads();
    const IcpGridHdr h = sh.hdr;
    const uint32_t *goff = w.cell_off + (size_t)pb.tgt_slot * (kIcpCells + 1);
    for (int c = tid; c <= h.nx * h.ny; c += kIcpThreads) sh.off[c] = goff[c];
    reg_start(sh.loop, pb.guess, n_src, IcpRows{src}, cur);
    __syncthreads();
    const double D2 = prm.max_correspondence_distance * prm.max_correspondence_distance;
    double prev = 1.7976931348623157e308; /* DBL_MAX (thread 0's copy is the one used) */
    while (true) {
        reg_pass<0, 28>(sh.sums, n_src, [&](uint32_t i, float *, double *t) -> bool {
            const float4 s = cur[i];
            if (!finite3(s.x, s.y, s.z)) return false;
            float d;
            uint32_t j;
            if (!icp_nn(h, sh.off, tpts, s.x, s.y, s.z, D2, d, j) || !((double)d <= D2)) return false;
            const float4 tp = *reinterpret_cast<const float4 *>(tgt + (size_t)j * 12);
            const float4 tn = *reinterpret_cast<const float4 *>(tgt + (size_t)j * 12 + 4);
            const float nx = tn.x, ny = tn.y, nz = tn.z;
            if (finite3(nx, ny, nz)) {
                const float a = nz * s.y - ny * s.z, b = nx * s.z - nz * s.x, c = ny * s.x - nx * s.y;
                const float dd = ((((nx * tp.x + ny * tp.y) + nz * tp.z) - nx * s.x) - ny * s.y) - nz * s.z;
                const double r[6] = {a, b, c, nx, ny, nz};
                int k = 0;
#pragma unroll
                for (int u = 0; u < 6; ++u)
#pragma unroll
                    for (int v = u; v < 6; ++v) t[k++] = r[u] * r[v];
#pragma unroll
                for (int u = 0; u < 6; ++u) t[21 + u] = r[u] * (double)dd;
            }
            t[27] = (double)d;
            return true;
        });
        if (tid == 0) {
            if (sh.sums.cnt < 3) sh.loop.state = 5; /* NO_CORRESPONDENCES */
            else icp_step(sh, prm, prev);
        }
        __syncthreads();
        if (sh.loop.state != 0) break;
        reg_advance(sh.loop, n_src, cur);
    }
    reg_finish(sh.sums, sh.loop, n_src, IcpRows{src}, h, sh.off, tpts, results + pb.result);
}

__global__ void k_icp_best(const bev_icp_result_t *res, int n_matches, int32_t *best)
{
    const int m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m < n_matches) best[m] = res[2 * m].fitness < res[2 * m + 1].fitness ? 0 : 1;
}

void launch_icp_grid(const float *pn, size_t stride, const uint32_t *counts, const uint32_t *slot_frame, int n_slots,
                     const IcpWork &w, hipStream_t st)
{
    if (n_slots > 0) hipLaunchKernelGGL(k_icp_grid, dim3(n_slots), dim3(kIcpThreads), 0, st, pn, stride, counts, slot_frame, w);
}

void launch_icp(const float *pn, size_t stride, const uint32_t *counts, const IcpProblem *probs, int n,
                const IcpWork &w, const bev_icp_params_t &prm, bev_icp_result_t *results, hipStream_t st)
{
    if (n > 0) hipLaunchKernelGGL(k_icp, dim3(n), dim3(kIcpThreads), 0, st, pn, stride, counts, probs, w, prm, results);
}

void launch_icp_best(const bev_icp_result_t *res, int n_matches, int32_t *best, hipStream_t st)
{
    if (n_matches > 0) hipLaunchKernelGGL(k_icp_best, dim3((n_matches + 255) / 256), dim3(256), 0, st, res, n_matches, best);
}

} /* namespace bevk */
