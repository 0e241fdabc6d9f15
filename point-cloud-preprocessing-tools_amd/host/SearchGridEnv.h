/*
 * SearchGridEnv.h — the text of BEV_SUBMAP_SEARCH_GRID (batch_submap_registration_main.cpp) and of
 * BEV_PAIR_SEARCH_GRID (batch_registration_main.cpp): "<fine>[,<coarse>]", the caps of cells per axis of the
 * search grids of the fine and the coarse stage.  The front ends print their own messages.
 */
#ifndef SEARCH_GRID_ENV_H
#define SEARCH_GRID_ENV_H

#include <cstdlib>

/* "<fine>[,<coarse>]": one or two integers 0 ... max and nothing else; one number sets both */
inline bool parse_search_grid(const char *s, long max, int dims[2])
{
    for (int k = 0; k < 2; ++k) {
        if (*s < '0' || *s > '9') return false; /* (strtol would take a sign or blanks) */
        char *end = nullptr;
        const long v = std::strtol(s, &end, 10);
        if (v > max) return false;
        dims[k] = (int)v;
        if (*end == '\0') {
            if (k == 0) dims[1] = dims[0];
            return true;
        }
        if (*end != ',' || k == 1) return false;
        s = end + 1;
    }
    return false;
}

#endif /* SEARCH_GRID_ENV_H */
