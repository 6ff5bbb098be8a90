/*
 * profile_check.c - the conserved core of a profile (csrc/host/sat_profile.c) as a stand-alone program:
 * tests/test_profile_cpu.py builds this file and sat_profile.c twice, plainly and with gcc -fsanitize=address,undefined,
 * runs both on the same cases and compares what they print.  stdin holds one case after the other,
 *     n1 hits fraction
 *     n1 * n1 counts, row-major
 * and for each case one line goes out: the return value, joint_min and the n1 flags.  The arrays are allocated at
 * exactly their sizes, so that a read or write past either end is the sanitizer's to report.
 */
#include <stdio.h>
#include <stdlib.h>

#include "sat_profile.h"

int main(void)
{
    int n1;
    unsigned hits;
    double fraction;
    long cases = 0;
    while (scanf("%d %u %lf", &n1, &hits, &fraction) == 3) {
        if (n1 < 1 || n1 > 4096) {
            fprintf(stderr, "profile_check: case %ld: bad n1 %d\n", cases, n1);
            return 2;
        }
        uint32_t *joint = malloc(sizeof *joint * (size_t)n1 * (size_t)n1);
        uint8_t *in_core = malloc((size_t)n1);
        if (!joint || !in_core)
            return 2;
        for (size_t i = 0; i < (size_t)n1 * (size_t)n1; i++)
            if (scanf("%u", &joint[i]) != 1) {
                fprintf(stderr, "profile_check: case %ld: short matrix\n", cases);
                return 2;
            }
        for (int i = 0; i < n1; i++)
            in_core[i] = 0xEE;
        uint32_t least = 0xEEEEEEEEu;
        const int size = sat_profile_core(n1, hits, joint, fraction, in_core, &least);
        printf("%d %u", size, size < 0 ? 0u : least);
        for (int i = 0; size >= 0 && i < n1; i++)
            printf(" %d", in_core[i]);
        printf("\n");
        /* joint_min may be NULL; the answer is the same */
        if (sat_profile_core(n1, hits, joint, fraction, in_core, NULL) != size) {
            fprintf(stderr, "profile_check: case %ld: another size without joint_min\n", cases);
            return 1;
        }
        free(joint);
        free(in_core);
        cases++;
    }
    /* the null arrays */
    uint32_t one = 1;
    uint8_t flag = 0;
    if (sat_profile_core(1, 1, NULL, 0.5, &flag, NULL) != -1 || sat_profile_core(1, 1, &one, 0.5, NULL, NULL) != -1 ||
        sat_profile_core(0, 1, &one, 0.5, &flag, NULL) != -1) {
        fprintf(stderr, "profile_check: a bad argument was accepted\n");
        return 1;
    }
    printf("profile_check: %ld cases\n", cases);
    return 0;
}
