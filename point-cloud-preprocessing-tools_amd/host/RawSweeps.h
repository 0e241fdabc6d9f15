/*
 * RawSweeps.h — the file-reading half of the three selectors' extractPointCloud (MulranPointCloudSelect.cpp:105-131,
 * OxfordPointCloudSelect.cpp:155-198, KittiPointCloudSelect.cpp:166-184): a raw sweep file as the floats
 * bev_process_batch_xyzi / bev_project_device_resident take.  The row / column assignment that follows in the
 * reference runs on the GPU (include/bev_mi355x.h, "Range-image projection").
 *
 * MulRan / KITTI: records of four little-endian float32 (x, y, z, intensity); n = min(file size / 16, cap) with
 * cap = 64 * 1024 (MulRan, :113) or 64 * 2083 (KITTI, :174); a trailing partial record is ignored.
 * Oxford: n = file size / 16 (:162-169); four planes x[n] y[n] z[n] intensity[n] from the start of the file.
 *
 * Not reproduced: the reference's `while (!file.eof() && k < cap)` loop runs once more after the last complete record of a
 * file with fewer than cap records and pushes a point whose coordinates were never read — indeterminate values, undefined
 * behaviour.
 */
#ifndef BEV_HOST_RAWSWEEPS_H
#define BEV_HOST_RAWSWEEPS_H

#include <cstddef>
#include <string>
#include <vector>

#include "Utility.h"

/* the values of BEV_PROJECT_MULRAN_OS1_64 / _OXFORD_HDL_32E / _KITTI_HDL_64E */
enum RawFormat { RAW_MULRAN = 0, RAW_OXFORD = 1, RAW_KITTI = 2, RAW_UNKNOWN = -1 };

RawFormat parseRawFormat(const std::string &name); /* "mulran", "oxford", "kitti" */
/* the sensor whose range image the format's projection fills: mulran <-> OS1_64, oxford <-> HDL_32E, kitti <-> HDL_64E */
bool rawFormatFitsSensor(RawFormat format, SensorType sensor);
/* returns a file of `file_bytes` bytes holds for the format (the caps above) */
std::size_t rawSweepReturns(RawFormat format, std::size_t file_bytes);
/* out: 4 * n floats, as the format's projection takes them.  false: the file cannot be opened or read (out is empty) */
bool readRawSweep(RawFormat format, const std::string &path, std::vector<float> &out);
/* the files of a directory whose name ends in .<ext>, sorted (getPcdFileNames, BatchMultiBevGen.cpp:469-494, for any
 * extension) */
void getFileNamesWithExtension(std::string path, const std::string &ext, std::vector<std::string> &filenames);

#endif
