/*
 * Registration.h — the front end of the reference's registration tools (top_part_registration,
 * batch_top_part_registration, batch_whole_registration), reference-named callers over the C ABI, one call each:
 *   extractTopAndFlatten   TopPartRegistration.cpp:79-136 (= BatchTopPartRegistration.cpp:90-147)
 *   VoxelGridXYZ           pcl::VoxelGrid<pcl::PointXYZ> (BatchTopPartRegistration.cpp:342-343,405-409)
 *   Normal2dEstimation     src/Normal2dEstimation.cpp (radius mode), src/PCA2D.cpp
 *   addNormal              BatchTopPartRegistration.cpp:155-172 (radius 2, viewpoint at the origin, concatenateFields)
 * and the coarse registration the front end feeds:
 *   MatchResult, IcpAlignResult, loadMatchResults   BatchTopPartRegistration.cpp:76-88, 250-272 (MatchResults.cpp: no
 *                                                   device code, so a plain g++ build can use it)
 *   performCoarseIcp       :192-221 (IterativeClosestPointWithNormals, D = 10, 10 iterations)
 *   coarseRegisterMatches  the tool's loop (:415-466): both yaw guesses of every match and the better one, in one batch
 * and the fine stage both batch tools end with:
 *   VoxelGridXYZIRCT       pcl::VoxelGrid<pcl::PointXYZIRCT> (:345-346, 483-487)
 *   performFineIcp         :224-247 (IterativeClosestPoint<PointXYZIRCT, PointXYZIRCT>, SVD; the top-part tool's
 *                          settings by default, the whole tool's through bev_icp_whole_defaults())
 *   fineRegisterMatches    the voxel grids and the fine ICP of every match in one batch (:480-497; the whole tool,
 *                          BatchWholeRegistration.cpp:372-389, from the yaw guess)
 *   rotationMatrixToEulerAngles  :290-309
 * The contracts are DESIGN.md "Registration front end" (§6b), "Coarse ICP" (§6c) and "Fine ICP" (§6d).
 */
#ifndef BEV_HOST_REGISTRATION_H
#define BEV_HOST_REGISTRATION_H

#include <array>
#include <stdexcept>
#include <string>

#include "PointCloud.h"

void extractTopAndFlatten(pcl::PointCloud<pcl::PointXYZIRCT>::Ptr &cloud_input,
                          pcl::PointCloud<pcl::PointXYZ>::Ptr &cloud_output);

/* pcl::VoxelGrid<pcl::PointXYZ>: setInputCloud, setLeafSize (one size for x, y, z), filter */
class VoxelGridXYZ {
public:
    void setInputCloud(const pcl::PointCloud<pcl::PointXYZ>::Ptr &cloud) { m_in = cloud; }
    void setLeafSize(float lx, float ly, float lz);
    void filter(pcl::PointCloud<pcl::PointXYZ> &output) const;

private:
    pcl::PointCloud<pcl::PointXYZ>::Ptr m_in;
    float m_leaf = 0.0f;
};

class Normal2dEstimation {
public:
    void setInputCloud(const pcl::PointCloud<pcl::PointXYZ>::Ptr &cloud) { m_in = cloud; }
    void setRadiusSearch(double radius) { m_radius = radius; }
    void setKSearch(int k) { m_k = k; } /* compute() then fails: k-search is not built */
    void setViewPoint(float vpx, float vpy, float vpz)
    {
        m_vp[0] = vpx;
        m_vp[1] = vpy;
        m_vp[2] = vpz;
    }
    /* throws std::runtime_error like the reference for a missing / double search setting, and for any library error */
    void compute(const pcl::PointCloud<pcl::Normal>::Ptr &normals) const;

private:
    pcl::PointCloud<pcl::PointXYZ>::Ptr m_in;
    double m_radius = 0.0;
    int m_k = 0;
    float m_vp[3] = {0.0f, 0.0f, 0.0f};
};

void addNormal(pcl::PointCloud<pcl::PointXYZ>::Ptr cloud, pcl::PointCloud<pcl::PointNormal>::Ptr cloud_with_normals);

struct MatchResult {
    int32_t query_idx; /* the source frame */
    int32_t match_idx; /* the target frame */
    float angle_guess; /* degrees */
};
static_assert(sizeof(MatchResult) == sizeof(bev_match_t), "MatchResult must match bev_match_t");

struct IcpAlignResult {
    bool is_converged = false;
    double fitness_score = 0.0;
    std::array<float, 16> final_transformation{}; /* row-major 4 x 4 (Eigen::Matrix4f in the reference) */
    int iterations = 0;
    int state = 0; /* BEV_ICP_* */
};

/* one "query match angle" triple per line (whitespace separated); a blank line is skipped (the reference would push an
 * uninitialised entry), a line that does not hold the three numbers throws std::runtime_error, as does a file that cannot
 * be opened (the reference exits) */
std::vector<MatchResult> loadMatchResults(std::string match_results_filename);

/* IterativeClosestPointWithNormals with D = 10 and 10 iterations from initial_guess (row-major); src_aligned (may be
 * null) receives the source moved by the final transformation (points by Transformer::se3, normals by its rotation) */
IcpAlignResult performCoarseIcp(pcl::PointCloud<pcl::PointNormal>::Ptr &points_with_normals_src,
                                pcl::PointCloud<pcl::PointNormal>::Ptr &points_with_normals_tgt,
                                pcl::PointCloud<pcl::PointNormal>::Ptr points_with_normals_src_aligned,
                                const std::array<float, 16> &initial_guess);

struct CoarseMatch {
    IcpAlignResult results[2]; /* from angle_guess and angle_guess + 180 */
    int best = 1;              /* 0 iff results[0].fitness_score < results[1].fitness_score */
};
/* the tool's coarse loop over every match at once: clouds[f] is frame f's PointNormal cloud (addNormal's output) */
std::vector<CoarseMatch> coarseRegisterMatches(const std::vector<pcl::PointCloud<pcl::PointNormal>::Ptr> &clouds,
                                               const std::vector<MatchResult> &matches);

/* pcl::VoxelGrid<pcl::PointXYZIRCT>: setInputCloud, setLeafSize (one size for x, y, z), filter */
class VoxelGridXYZIRCT {
public:
    void setInputCloud(const pcl::PointCloud<pcl::PointXYZIRCT>::Ptr &cloud) { m_in = cloud; }
    void setLeafSize(float lx, float ly, float lz);
    void filter(pcl::PointCloud<pcl::PointXYZIRCT> &output) const;

private:
    pcl::PointCloud<pcl::PointXYZIRCT>::Ptr m_in;
    float m_leaf = 0.0f;
};

/* IterativeClosestPoint<PointXYZIRCT, PointXYZIRCT> from initial_guess (row-major) with params (the top-part tool's: D 1,
 * 1e-6, 0.01, 100 iterations); full_cloud_1_ds_aligned (may be null) receives the source moved by the final
 * transformation (Transformer::se3) */
IcpAlignResult performFineIcp(pcl::PointCloud<pcl::PointXYZIRCT>::Ptr &full_cloud_1_ds,
                              pcl::PointCloud<pcl::PointXYZIRCT>::Ptr &full_cloud_2_ds,
                              pcl::PointCloud<pcl::PointXYZIRCT>::Ptr full_cloud_1_ds_aligned,
                              const std::array<float, 16> &initial_guess,
                              const bev_icp_params_t &params = bev_icp_fine_defaults());

/* the fine stage of every match at once: clouds[f] is frame f's full labelled cloud (null: empty); the voxel grid (leaf)
 * of every frame named, then ICP from coarse[m]'s better result (the top-part tool) or, with coarse null, from the yaw
 * guess angle_guess (the whole tool) */
std::vector<IcpAlignResult> fineRegisterMatches(const std::vector<pcl::PointCloud<pcl::PointXYZIRCT>::Ptr> &clouds,
                                                const std::vector<MatchResult> &matches,
                                                const std::vector<CoarseMatch> *coarse, const bev_icp_params_t &params,
                                                float leaf = 0.2f);

/* rotationMatrixToEulerAngles (:290-309) on a row-major 3 x 3, in float with the host libm: (x, y, z) */
std::array<float, 3> rotationMatrixToEulerAngles(const std::array<float, 9> &R);

/* (diff_xy, diff_yaw) of a successful match's report line (BatchTopPartRegistration.cpp:512-527): the fine transform Tf
 * against the transform Tc it started from (row-major 4 x 4), in float with the host libm */
void icpPrecisionReport(const float *Tf, const float *Tc, float &diff_xy, float &diff_yaw);

#endif
