/*
 * sat_profile.h - the conserved core of a query's profile (-W P, sat_profile_rows of include/satabsearch.h).
 *
 * A profile of a query of n1 SSEs: hits, the rows that counted, and joint[n1][n1], row-major, full and symmetric:
 * joint[i][k] = the counted rows whose map matches SSE i and SSE k, joint[i][i] = those that match SSE i at all (so
 * joint[i][k] <= min(joint[i][i], joint[k][k])).  The core is a set of SSEs that are matched TOGETHER: with
 * t = fraction * hits, every comparison made in double,
 *     1. S = { i : joint[i][i] >= t }
 *     2. among the pairs i < k of S with joint[i][k] < t take one with the smallest joint[i][k], ties to the smallest i,
 *        then the smallest k; none: stop
 *     3. drop the member of that pair with the smaller diagonal count, ties dropping the larger index; go to 2
 * Every two SSEs of the result are matched together in at least `fraction` of the hits.
 */
#ifndef SAT_PROFILE_H
#define SAT_PROFILE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/*
 * in_core[i] = 1 for the SSEs of the core, else 0; *joint_min (may be NULL) = the smallest joint count among the pairs
 * of the core, the diagonal count when the core is one SSE, 0 when it is empty.  Returns the size of the core - 0 for
 * hits == 0 or an empty S - or -1 on a bad argument: n1 < 1, a null array, fraction outside (0, 1] (a NaN included).
 */
int sat_profile_core(int n1, uint32_t hits, const uint32_t *joint, double fraction, uint8_t *in_core, uint32_t *joint_min);

#ifdef __cplusplus
}
#endif
#endif
