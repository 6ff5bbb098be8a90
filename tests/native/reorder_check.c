/*
 * reorder_check.c - the order of a solution map (csrc/host/sat_reorder.c) as a stand-alone program:
 * tests/test_reorder_cpu.py builds this file and sat_reorder.c twice, plainly and with gcc -fsanitize=address,undefined,
 * runs both on the same maps and compares what they print.  stdin holds one map a line,
 *     n1 m_0 .. m_(n1-1)
 * and for each one line goes out: kind matched descents cut.  The map is allocated at exactly its size, so that a read
 * past either end is the sanitizer's to report.
 */
#include <stdio.h>
#include <stdlib.h>

#include "sat_reorder.h"

int main(void)
{
    int n1;
    long maps = 0;
    while (scanf("%d", &n1) == 1) {
        if (n1 < 0 || n1 > 4096) {
            fprintf(stderr, "reorder_check: map %ld: bad n1 %d\n", maps, n1);
            return 2;
        }
        int32_t *map = n1 ? malloc(sizeof *map * (size_t)n1) : NULL;
        if (n1 && !map)
            return 2;
        for (int i = 0; i < n1; i++)
            if (scanf("%d", &map[i]) != 1) {
                fprintf(stderr, "reorder_check: map %ld: short map\n", maps);
                return 2;
            }
        int32_t matched = 0xEEEE, descents = 0xEEEE, cut = 0xEEEE;
        const int32_t kind = sat_map_kind(map, n1, &matched, &descents, &cut);
        printf("%d %d %d %d\n", kind, matched, descents, cut);
        /* the outputs may be NULL; the answer is the same */
        if (sat_map_kind(map, n1, NULL, NULL, NULL) != kind) {
            fprintf(stderr, "reorder_check: map %ld: another kind without the outputs\n", maps);
            return 1;
        }
        free(map);
        maps++;
    }
    int32_t one = 0;
    if (sat_map_kind(NULL, 1, NULL, NULL, NULL) != -1 || sat_map_kind(&one, -1, NULL, NULL, NULL) != -1 ||
        sat_map_kind(NULL, 0, NULL, NULL, NULL) != SAT_KIND_SEQUENTIAL) {
        fprintf(stderr, "reorder_check: a bad argument was accepted\n");
        return 1;
    }
    printf("reorder_check: %ld maps\n", maps);
    return 0;
}
