/* sat_eval.c - see sat_eval.h */
#include "sat_eval.h"

#include <stddef.h>

int sat_eval_reduce(const uint32_t *pos, const uint32_t *neg, int32_t bins, int32_t rocn, sat_eval_row *out)
{
    if (!pos || !neg || !out || bins < 1 || rocn < 1)
        return -1;
    uint64_t np = 0, nn = 0;
    for (int32_t b = 0; b < bins; b++) {
        np += pos[b];
        nn += neg[b];
    }
    if (np > 0x7FFFFFFFu || nn > 0x7FFFFFFFu)
        return -1;
    out->u2 = out->t2 = 0;
    out->positives = out->negatives = out->n_used = 0;
    sat_eval_walk(out, pos, neg, bins, rocn);
    return 0;
}
