/*
 * Registration.h — the front end of the reference's registration tools (top_part_registration,
 * batch_top_part_registration, batch_whole_registration), reference-named callers over the C ABI, one call each:
 *   extractTopAndFlatten   TopPartRegistration.cpp:79-136 (= BatchTopPartRegistration.cpp:90-147)
 *   VoxelGridXYZ           pcl::VoxelGrid<pcl::PointXYZ> (BatchTopPartRegistration.cpp:342-343,405-409)
 *   Normal2dEstimation     src/Normal2dEstimation.cpp (radius mode), src/PCA2D.cpp
 *   addNormal              BatchTopPartRegistration.cpp:155-172 (radius 2, viewpoint at the origin, concatenateFields)
 * The contract is DESIGN.md "Registration front end".  ICP is not here.
 */
#ifndef BEV_HOST_REGISTRATION_H
#define BEV_HOST_REGISTRATION_H

#include <stdexcept>

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

#endif
