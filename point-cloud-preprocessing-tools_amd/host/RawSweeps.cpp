#include "RawSweeps.h"

#include <dirent.h>
#include <sys/stat.h>

#include <algorithm>
#include <cstdio>
#include <iostream>

RawFormat parseRawFormat(const std::string &name)
{
    if (name == "mulran") return RAW_MULRAN;
    if (name == "oxford") return RAW_OXFORD;
    if (name == "kitti") return RAW_KITTI;
    return RAW_UNKNOWN;
}

bool rawFormatFitsSensor(RawFormat format, SensorType sensor)
{
    return (format == RAW_MULRAN && sensor == OS1_64) || (format == RAW_OXFORD && sensor == HDL_32E) ||
           (format == RAW_KITTI && sensor == HDL_64E);
}

std::size_t rawSweepReturns(RawFormat format, std::size_t file_bytes)
{
    const std::size_t n = file_bytes / 16;
    if (format == RAW_MULRAN) return std::min<std::size_t>(n, 64 * 1024); /* MAX_NUM_POINTS, MulranPointCloudSelect.cpp:113 */
    if (format == RAW_KITTI) return std::min<std::size_t>(n, 64 * 2083);  /* KittiPointCloudSelect.cpp:174 */
    return format == RAW_OXFORD ? n : 0;                                  /* OxfordPointCloudSelect.cpp:169 */
}

bool readRawSweep(RawFormat format, const std::string &path, std::vector<float> &out)
{
    static_assert(sizeof(float) == 4, "float32 records");
    out.clear();
    if (format == RAW_UNKNOWN) return false;
    struct stat st;
    if (stat(path.c_str(), &st) != 0 || !S_ISREG(st.st_mode)) return false;
    FILE *f = std::fopen(path.c_str(), "rb");
    if (!f) return false;
    const long long size = (long long)st.st_size;
    bool ok = true;
    {
        /* (x86-64 and the file are little-endian: the bytes are the floats.  Oxford's planes are n floats apart from the
         * start of the file, so the first 4 n floats are the four planes whatever follows them) */
        const std::size_t n = rawSweepReturns(format, (std::size_t)size);
        out.resize(4 * n);
        ok = n == 0 || std::fread(out.data(), 16, n, f) == n;
    }
    std::fclose(f);
    if (!ok) out.clear();
    return ok;
}

void getFileNamesWithExtension(std::string path, const std::string &ext, std::vector<std::string> &filenames)
{
    DIR *dir = opendir(path.c_str());
    if (!dir) {
        std::cerr << "Folder doesn't Exist!" << std::endl; /* :473-476 */
        return;
    }
    while (dirent *e = readdir(dir)) {
        const std::string name = e->d_name;
        const size_t dot = name.find_last_of('.');
        if (name.substr(dot + 1) != ext) continue; /* :482-484 (also drops "." and "..") */
        filenames.push_back(path.back() == '/' ? path + name : path + "/" + name);
    }
    closedir(dir);
    std::sort(filenames.begin(), filenames.end()); /* :493 */
}
