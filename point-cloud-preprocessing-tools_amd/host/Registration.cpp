/* Registration.cpp — see Registration.h.  Every computation happens behind the C ABI (bev_regfront.h, bev_icp.h on the
 * GPU); only performCoarseIcp's aligned copy of the source is moved on the host. */
#include "Registration.h"

#include <algorithm>
#include <cmath>
#include <string>

#include <hip/hip_runtime_api.h>

bev_ctx_t *bevhost_context(); /* BatchMultiBevGen.cpp (host): the lazily created context of the free functions */

static void check(int rc, const char *what)
{
    if (rc != BEV_OK) throw std::runtime_error(std::string(what) + ": " + bev_strerror(rc));
}

void extractTopAndFlatten(pcl::PointCloud<pcl::PointXYZIRCT>::Ptr &cloud_input,
                          pcl::PointCloud<pcl::PointXYZ>::Ptr &cloud_output)
{
    const uint32_t n = (uint32_t)cloud_input->points.size();
    std::vector<pcl::PointXYZ> out(bev_regfront_max_out(n));
    uint32_t m = 0;
    check(bev_top_part_flatten(bevhost_context(), reinterpret_cast<const bev_point_t *>(cloud_input->points.data()), n,
                               reinterpret_cast<float *>(out.data()), &m),
          "extractTopAndFlatten");
    for (uint32_t i = 0; i < m; ++i) cloud_output->push_back(out[i]); /* (appends, like the reference) */
}

void VoxelGridXYZ::setLeafSize(float lx, float ly, float lz)
{
    if (lx != ly || ly != lz) throw std::runtime_error("VoxelGridXYZ: one leaf size for x, y and z");
    m_leaf = lx;
}

void VoxelGridXYZ::filter(pcl::PointCloud<pcl::PointXYZ> &output) const
{
    if (!m_in) throw std::runtime_error("VoxelGridXYZ: no input cloud");
    const uint32_t n = (uint32_t)m_in->points.size();
    std::vector<pcl::PointXYZ> out(n ? n : 1);
    uint32_t m = 0;
    check(bev_voxel_grid_xyz(bevhost_context(), reinterpret_cast<const float *>(m_in->points.data()), n, m_leaf,
                             reinterpret_cast<float *>(out.data()), &m),
          "VoxelGrid::filter");
    output.resize(m);
    std::copy(out.begin(), out.begin() + m, output.points.begin());
}

void Normal2dEstimation::compute(const pcl::PointCloud<pcl::Normal>::Ptr &normals) const
{
    if (m_k == 0 && m_radius == 0) throw std::runtime_error("You must call once either setRadiusSearch or setKSearch !");
    if (m_k != 0 && m_radius != 0)
        throw std::runtime_error("You must call once either setRadiusSearch or setKSearch (not both) !");
    if (!m_in) throw std::runtime_error("Normal2dEstimation: no input cloud");
    const uint32_t n = (uint32_t)m_in->points.size();
    normals->resize(n);
    normals->width = m_in->width;
    normals->height = m_in->height;
    check(bev_normals_2d(bevhost_context(), reinterpret_cast<const float *>(m_in->points.data()), n, m_k, (float)m_radius,
                         m_vp, reinterpret_cast<float *>(normals->points.data())),
          "Normal2dEstimation::compute");
}

void addNormal(pcl::PointCloud<pcl::PointXYZ>::Ptr cloud, pcl::PointCloud<pcl::PointNormal>::Ptr cloud_with_normals)
{
    pcl::PointCloud<pcl::Normal>::Ptr normals(new pcl::PointCloud<pcl::Normal>());
    Normal2dEstimation norm_est;
    norm_est.setInputCloud(cloud);
    norm_est.setRadiusSearch(2);
    norm_est.compute(normals);
    /* pcl::concatenateFields */
    const size_t n = cloud->points.size();
    cloud_with_normals->resize(n);
    for (size_t i = 0; i < n; ++i) {
        pcl::PointNormal &o = cloud_with_normals->points[i];
        o = pcl::PointNormal{};
        o.x = cloud->points[i].x;
        o.y = cloud->points[i].y;
        o.z = cloud->points[i].z;
        o.normal_x = normals->points[i].normal_x;
        o.normal_y = normals->points[i].normal_y;
        o.normal_z = normals->points[i].normal_z;
        o.curvature = normals->points[i].curvature;
    }
}

/* ---- coarse ICP ------------------------------------------------------------------------------------------------------ */
static IcpAlignResult to_align_result(const bev_icp_result_t &r)
{
    IcpAlignResult a;
    a.is_converged = r.converged != 0;
    a.fitness_score = r.fitness;
    std::copy(r.T, r.T + 16, a.final_transformation.begin());
    a.iterations = r.iterations;
    a.state = r.state;
    return a;
}

IcpAlignResult performCoarseIcp(pcl::PointCloud<pcl::PointNormal>::Ptr &points_with_normals_src,
                                pcl::PointCloud<pcl::PointNormal>::Ptr &points_with_normals_tgt,
                                pcl::PointCloud<pcl::PointNormal>::Ptr points_with_normals_src_aligned,
                                const std::array<float, 16> &initial_guess)
{
    const bev_icp_params_t prm = bev_icp_coarse_defaults();
    bev_icp_result_t r{};
    const auto &src = points_with_normals_src->points;
    const auto &tgt = points_with_normals_tgt->points;
    check(bev_icp_point_to_plane(bevhost_context(), reinterpret_cast<const float *>(src.data()), (uint32_t)src.size(),
                                 reinterpret_cast<const float *>(tgt.data()), (uint32_t)tgt.size(), initial_guess.data(),
                                 &prm, &r),
          "performCoarseIcp");
    if (points_with_normals_src_aligned) {
        const float *T = r.T;
        points_with_normals_src_aligned->resize(src.size());
        for (size_t i = 0; i < src.size(); ++i) {
            pcl::PointNormal o = src[i];
            const float x = o.x, y = o.y, z = o.z, nx = o.normal_x, ny = o.normal_y, nz = o.normal_z;
            o.x = T[0] * x + (T[1] * y + (T[2] * z + T[3]));
            o.y = T[4] * x + (T[5] * y + (T[6] * z + T[7]));
            o.z = T[8] * x + (T[9] * y + (T[10] * z + T[11]));
            o.normal_x = (T[0] * nx + T[1] * ny) + T[2] * nz;
            o.normal_y = (T[4] * nx + T[5] * ny) + T[6] * nz;
            o.normal_z = (T[8] * nx + T[9] * ny) + T[10] * nz;
            points_with_normals_src_aligned->points[i] = o;
        }
    }
    return to_align_result(r);
}

std::vector<CoarseMatch> coarseRegisterMatches(const std::vector<pcl::PointCloud<pcl::PointNormal>::Ptr> &clouds,
                                               const std::vector<MatchResult> &matches)
{
    std::vector<CoarseMatch> out(matches.size());
    if (matches.empty()) return out;
    size_t stride = 1;
    for (const auto &cl : clouds) stride = std::max(stride, cl ? cl->points.size() : (size_t)0);
    const size_t F = clouds.size();
    std::vector<pcl::PointNormal> packed(F * stride);
    std::vector<uint32_t> counts(F, 0);
    for (size_t f = 0; f < F; ++f) {
        if (!clouds[f]) continue;
        std::copy(clouds[f]->points.begin(), clouds[f]->points.end(), packed.begin() + f * stride);
        counts[f] = (uint32_t)clouds[f]->points.size();
    }
    void *d_pn = nullptr, *d_counts = nullptr, *d_res = nullptr, *d_best = nullptr;
    auto release = [&]() {
        for (void *p : {d_pn, d_counts, d_res, d_best})
            if (p) (void)hipFree(p);
    };
    auto hip = [&](hipError_t e, const char *what) {
        if (e != hipSuccess) {
            release();
            throw std::runtime_error(std::string("coarseRegisterMatches: ") + what + ": " + hipGetErrorString(e));
        }
    };
    bev_ctx_t *ctx = bevhost_context();
    hip(hipMalloc(&d_pn, packed.size() * sizeof(pcl::PointNormal)), "hipMalloc");
    hip(hipMalloc(&d_counts, F * 4), "hipMalloc");
    hip(hipMalloc(&d_res, matches.size() * 2 * sizeof(bev_icp_result_t)), "hipMalloc");
    hip(hipMalloc(&d_best, matches.size() * 4), "hipMalloc");
    hip(hipMemcpy(d_pn, packed.data(), packed.size() * sizeof(pcl::PointNormal), hipMemcpyHostToDevice), "hipMemcpy");
    hip(hipMemcpy(d_counts, counts.data(), F * 4, hipMemcpyHostToDevice), "hipMemcpy");
    int rc = bev_coarse_registration_device_resident(ctx, (int)F, d_pn, stride, static_cast<uint32_t *>(d_counts),
                                                     (int)matches.size(),
                                                     reinterpret_cast<const bev_match_t *>(matches.data()), nullptr,
                                                     static_cast<bev_icp_result_t *>(d_res), static_cast<int32_t *>(d_best));
    if (rc == BEV_OK) rc = bev_synchronize(ctx);
    if (rc != BEV_OK) {
        release();
        check(rc, "coarseRegisterMatches");
    }
    std::vector<bev_icp_result_t> res(matches.size() * 2);
    std::vector<int32_t> best(matches.size());
    hip(hipMemcpy(res.data(), d_res, res.size() * sizeof(bev_icp_result_t), hipMemcpyDeviceToHost), "hipMemcpy");
    hip(hipMemcpy(best.data(), d_best, best.size() * 4, hipMemcpyDeviceToHost), "hipMemcpy");
    release();
    for (size_t m = 0; m < matches.size(); ++m) {
        out[m].results[0] = to_align_result(res[2 * m]);
        out[m].results[1] = to_align_result(res[2 * m + 1]);
        out[m].best = best[m];
    }
    return out;
}

/* ---- fine stage ------------------------------------------------------------------------------------------------------ */
void VoxelGridXYZIRCT::setLeafSize(float lx, float ly, float lz)
{
    if (lx != ly || ly != lz) throw std::runtime_error("VoxelGridXYZIRCT: one leaf size for x, y and z");
    m_leaf = lx;
}

void VoxelGridXYZIRCT::filter(pcl::PointCloud<pcl::PointXYZIRCT> &output) const
{
    const uint32_t n = m_in ? (uint32_t)m_in->points.size() : 0u;
    std::vector<pcl::PointXYZIRCT> out(std::max<uint32_t>(n, 1));
    uint32_t m = 0;
    check(bev_voxel_grid_irct(bevhost_context(), n ? reinterpret_cast<const bev_point_t *>(m_in->points.data()) : nullptr,
                              n, m_leaf, reinterpret_cast<bev_point_t *>(out.data()), &m),
          "VoxelGridXYZIRCT::filter");
    output.points.assign(out.begin(), out.begin() + m);
    output.width = m;
    output.height = 1;
}

IcpAlignResult performFineIcp(pcl::PointCloud<pcl::PointXYZIRCT>::Ptr &full_cloud_1_ds,
                              pcl::PointCloud<pcl::PointXYZIRCT>::Ptr &full_cloud_2_ds,
                              pcl::PointCloud<pcl::PointXYZIRCT>::Ptr full_cloud_1_ds_aligned,
                              const std::array<float, 16> &initial_guess, const bev_icp_params_t &params)
{
    bev_icp_result_t r{};
    const auto &src = full_cloud_1_ds->points;
    const auto &tgt = full_cloud_2_ds->points;
    check(bev_icp_point_to_point(bevhost_context(), reinterpret_cast<const bev_point_t *>(src.data()), (uint32_t)src.size(),
                                 reinterpret_cast<const bev_point_t *>(tgt.data()), (uint32_t)tgt.size(),
                                 initial_guess.data(), &params, &r),
          "performFineIcp");
    if (full_cloud_1_ds_aligned) {
        const float *T = r.T;
        full_cloud_1_ds_aligned->points.resize(src.size());
        for (size_t i = 0; i < src.size(); ++i) {
            pcl::PointXYZIRCT o = src[i];
            const float x = o.x, y = o.y, z = o.z;
            o.x = T[0] * x + (T[1] * y + (T[2] * z + T[3]));
            o.y = T[4] * x + (T[5] * y + (T[6] * z + T[7]));
            o.z = T[8] * x + (T[9] * y + (T[10] * z + T[11]));
            full_cloud_1_ds_aligned->points[i] = o;
        }
    }
    return to_align_result(r);
}

std::vector<IcpAlignResult> fineRegisterMatches(const std::vector<pcl::PointCloud<pcl::PointXYZIRCT>::Ptr> &clouds,
                                                const std::vector<MatchResult> &matches,
                                                const std::vector<CoarseMatch> *coarse, const bev_icp_params_t &params,
                                                float leaf)
{
    std::vector<IcpAlignResult> out(matches.size());
    if (matches.empty()) return out;
    if (coarse && coarse->size() != matches.size()) throw std::runtime_error("fineRegisterMatches: one coarse result per match");
    const size_t F = clouds.size();
    std::vector<uint64_t> offs(F + 1, 0);
    for (size_t f = 0; f < F; ++f) offs[f + 1] = offs[f] + (clouds[f] ? clouds[f]->points.size() : 0);
    void *d_pts = nullptr, *d_coarse = nullptr, *d_best = nullptr, *d_res = nullptr;
    auto release = [&]() {
        for (void *p : {d_pts, d_coarse, d_best, d_res})
            if (p) (void)hipFree(p);
    };
    auto hip = [&](hipError_t e, const char *what) {
        if (e != hipSuccess) {
            release();
            throw std::runtime_error(std::string("fineRegisterMatches: ") + what + ": " + hipGetErrorString(e));
        }
    };
    bev_ctx_t *ctx = bevhost_context();
    hip(hipMalloc(&d_pts, std::max<size_t>(offs[F], 1) * sizeof(bev_point_t)), "hipMalloc");
    for (size_t f = 0; f < F; ++f)
        if (offs[f + 1] > offs[f])
            hip(hipMemcpy(static_cast<bev_point_t *>(d_pts) + offs[f], clouds[f]->points.data(),
                          (offs[f + 1] - offs[f]) * sizeof(bev_point_t), hipMemcpyHostToDevice),
                "hipMemcpy");
    if (coarse) {
        std::vector<bev_icp_result_t> cr(matches.size() * 2);
        std::vector<int32_t> best(matches.size());
        for (size_t m = 0; m < matches.size(); ++m) {
            for (int g = 0; g < 2; ++g)
                std::copy((*coarse)[m].results[g].final_transformation.begin(),
                          (*coarse)[m].results[g].final_transformation.end(), cr[2 * m + g].T);
            best[m] = (*coarse)[m].best;
        }
        hip(hipMalloc(&d_coarse, cr.size() * sizeof(bev_icp_result_t)), "hipMalloc");
        hip(hipMalloc(&d_best, best.size() * 4), "hipMalloc");
        hip(hipMemcpy(d_coarse, cr.data(), cr.size() * sizeof(bev_icp_result_t), hipMemcpyHostToDevice), "hipMemcpy");
        hip(hipMemcpy(d_best, best.data(), best.size() * 4, hipMemcpyHostToDevice), "hipMemcpy");
    }
    hip(hipMalloc(&d_res, matches.size() * sizeof(bev_icp_result_t)), "hipMalloc");
    int rc = bev_fine_registration_device_resident(ctx, (int)F, static_cast<const bev_point_t *>(d_pts), offs.data(), leaf,
                                                   (int)matches.size(), reinterpret_cast<const bev_match_t *>(matches.data()),
                                                   static_cast<const bev_icp_result_t *>(d_coarse),
                                                   static_cast<const int32_t *>(d_best), &params,
                                                   static_cast<bev_icp_result_t *>(d_res));
    if (rc == BEV_OK) rc = bev_synchronize(ctx);
    if (rc != BEV_OK) {
        release();
        check(rc, "fineRegisterMatches");
    }
    std::vector<bev_icp_result_t> res(matches.size());
    hip(hipMemcpy(res.data(), d_res, res.size() * sizeof(bev_icp_result_t), hipMemcpyDeviceToHost), "hipMemcpy");
    release();
    for (size_t m = 0; m < matches.size(); ++m) out[m] = to_align_result(res[m]);
    return out;
}

/* (diff_xy, diff_yaw) of a successful match (BatchTopPartRegistration.cpp:512-527), in float with the host libm */
void icpPrecisionReport(const float *Tf, const float *Tc, float &diff_xy, float &diff_yaw)
{
    const float dx = Tf[3] - Tc[3], dy = Tf[7] - Tc[7];
    diff_xy = std::sqrt(dx * dx + dy * dy);
    float m[9], c[9];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) {
            m[i * 3 + j] = Tf[i * 4 + j];
            c[i * 3 + j] = Tc[i * 4 + j];
        }
    /* Eigen's cofactor inverse of a 3 x 3: result(r, k) = cofactor(k, r) / det */
    auto cof = [&](int i, int j) {
        const int i1 = (i + 1) % 3, i2 = (i + 2) % 3, j1 = (j + 1) % 3, j2 = (j + 2) % 3;
        return m[i1 * 3 + j1] * m[i2 * 3 + j2] - m[i1 * 3 + j2] * m[i2 * 3 + j1];
    };
    const float c00 = cof(0, 0), c10 = cof(1, 0), c20 = cof(2, 0);
    const float det = (c00 * m[0] + c10 * m[3]) + c20 * m[6];
    const float inv = 1.0f / det;
    const float Ri[9] = {c00 * inv, c10 * inv, c20 * inv, cof(0, 1) * inv, cof(1, 1) * inv,
                         cof(2, 1) * inv, cof(0, 2) * inv, cof(1, 2) * inv, cof(2, 2) * inv};
    std::array<float, 9> rel;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) rel[i * 3 + j] = (Ri[i * 3] * c[j] + Ri[i * 3 + 1] * c[3 + j]) + Ri[i * 3 + 2] * c[6 + j];
    const std::array<float, 3> e = rotationMatrixToEulerAngles(rel);
    diff_yaw = e[2] / M_PI * 180.0f;
    if (diff_yaw > 180.0f) diff_yaw -= 360.0f;
    if (diff_yaw < -180.0f) diff_yaw += 360.0f;
}
