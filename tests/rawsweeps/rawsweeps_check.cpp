/* C entry points over host/RawSweeps.h for the tests (tests/rawsweeps_lib.py). */
#include <cstring>
#include <string>
#include <vector>

#include "RawSweeps.h"

extern "C" {

int rs_parse_format(const char *name) { return (int)parseRawFormat(name ? name : ""); }

int rs_fits_sensor(int format, int sensor) { return rawFormatFitsSensor((RawFormat)format, (SensorType)sensor) ? 1 : 0; }

unsigned long long rs_returns(int format, unsigned long long file_bytes)
{
    return (unsigned long long)rawSweepReturns((RawFormat)format, (std::size_t)file_bytes);
}

/* the file's returns into out (room for cap floats); the number of floats, -1: unreadable, -2: more than cap */
long long rs_read(int format, const char *path, float *out, unsigned long long cap)
{
    std::vector<float> v;
    if (!readRawSweep((RawFormat)format, path, v)) return -1;
    if (v.size() > cap) return -2;
    if (!v.empty()) std::memcpy(out, v.data(), v.size() * sizeof(float));
    return (long long)v.size();
}

/* the sorted listing, names separated by '\n', into out (cap bytes, NUL-terminated); the number of files, -2: too long */
int rs_list(const char *dir, const char *ext, char *out, unsigned long long cap)
{
    std::vector<std::string> files;
    getFileNamesWithExtension(dir, ext, files);
    std::string all;
    for (const std::string &f : files) all += f + "\n";
    if (all.size() + 1 > cap) return -2;
    std::memcpy(out, all.c_str(), all.size() + 1);
    return (int)files.size();
}
}
