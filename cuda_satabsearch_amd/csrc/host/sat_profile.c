/* sat_profile.c - see sat_profile.h */
#include "sat_profile.h"

#include <stddef.h>

int sat_profile_core(int n1, uint32_t hits, const uint32_t *joint, double fraction, uint8_t *in_core, uint32_t *joint_min)
{
    if (n1 < 1 || !joint || !in_core || !(fraction > 0.0 && fraction <= 1.0))
        return -1;
    const double t = fraction * (double)hits;
    const size_t n = (size_t)n1;
    int size = 0;
    for (size_t i = 0; i < n; i++) {
        in_core[i] = hits > 0 && (double)joint[i * n + i] >= t;
        size += in_core[i];
    }
    /* every turn drops one member: n1 turns at most */
    for (;;) {
        size_t bi = n, bk = n;
        for (size_t i = 0; i < n; i++)
            for (size_t k = i + 1; in_core[i] && k < n; k++)
                if (in_core[k] && (double)joint[i * n + k] < t && (bi == n || joint[i * n + k] < joint[bi * n + bk])) {
                    bi = i;                     /* strictly smaller only: ties stay with the first pair in (i, k) order */
                    bk = k;
                }
        if (bi == n)
            break;
        in_core[joint[bi * n + bi] < joint[bk * n + bk] ? bi : bk] = 0;
        size--;
    }
    uint32_t least = 0;
    int first = 1;
    for (size_t i = 0; i < n; i++)
        for (size_t k = i + (size > 1); in_core[i] && k < n; k++)
            if (in_core[k] && (first || joint[i * n + k] < least)) {
                least = joint[i * n + k];
                first = 0;
            }
    if (joint_min)
        *joint_min = least;
    return size;
}
