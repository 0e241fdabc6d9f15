/* MatchResults.cpp — loadMatchResults (BatchTopPartRegistration.cpp:250-272): plain C++, no device code. */
#include <cmath>
#include <fstream>
#include <sstream>

#include "Registration.h"

std::vector<MatchResult> loadMatchResults(std::string match_results_filename)
{
    std::ifstream f_list(match_results_filename);
    if (!f_list.is_open()) throw std::runtime_error("Failed to open file: " + match_results_filename);
    std::vector<MatchResult> matches;
    std::string line;
    for (size_t line_no = 1; std::getline(f_list, line); ++line_no) {
        if (line.find_first_not_of(" \t\r") == std::string::npos) continue;
        std::stringstream ss(line);
        MatchResult m{};
        if (!(ss >> m.query_idx >> m.match_idx >> m.angle_guess))
            throw std::runtime_error(match_results_filename + ":" + std::to_string(line_no) +
                                     ": expected \"query_idx match_idx angle_guess\"");
        matches.push_back(m);
    }
    return matches;
}

/* rotationMatrixToEulerAngles (BatchTopPartRegistration.cpp:290-309): float, the host libm */
std::array<float, 3> rotationMatrixToEulerAngles(const std::array<float, 9> &R)
{
    const float sy = std::sqrt(R[0] * R[0] + R[3] * R[3]);
    if (!(sy < 1e-6)) return {std::atan2(R[7], R[8]), std::atan2(-R[6], sy), std::atan2(R[3], R[0])};
    return {std::atan2(-R[5], R[4]), std::atan2(-R[6], sy), 0.0f};
}
