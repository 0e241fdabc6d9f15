/* Registration.cpp — see Registration.h.  Every computation happens behind the C ABI (bev_regfront.h on the GPU). */
#include "Registration.h"

#include <algorithm>
#include <string>

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
