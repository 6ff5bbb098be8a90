/* sat_cluster.c - see sat_cluster.h */
#include "sat_cluster.h"

#include <stddef.h>

/* the root of v in a forest whose links only point to smaller nodes (p[v] <= v), halving the path on the way */
static int32_t find_root(int32_t *p, int32_t v)
{
    while (p[v] != v) {
        p[v] = p[p[v]];
        v = p[v];
    }
    return v;
}

int sat_cluster_join(int n, int nsets, const int32_t *labels, int32_t *out)
{
    if (n < 1 || nsets < 1 || !labels || !out)
        return -1;
    for (size_t i = 0; i < (size_t)nsets * (size_t)n; i++)
        if (labels[i] < 0 || labels[i] >= n)
            return -1;
    /* out is the forest: the larger root always goes under the smaller, so that a root is the smallest node of its tree */
    for (int32_t v = 0; v < n; v++)
        out[v] = v;
    for (int g = 0; g < nsets; g++)
        for (int32_t v = 0; v < n; v++) {
            const int32_t a = find_root(out, v), b = find_root(out, labels[(size_t)g * (size_t)n + v]);
            if (a < b)
                out[b] = a;
            else if (b < a)
                out[a] = b;
        }
    for (int32_t v = 0; v < n; v++)
        out[v] = find_root(out, v);
    return 0;
}

int sat_cluster_nested(int n, int n_levels, const int32_t *labels)
{
    if (n < 1 || n_levels < 1 || !labels)
        return -1;
    for (int j = 0; j < n_levels; j++) {
        const int32_t *label = labels + (size_t)j * (size_t)n;
        for (int32_t v = 0; v < n; v++)
            if (label[v] < 0 || label[v] > v || label[label[v]] != label[v])
                return -1;
    }
    /* level j refines level j + 1 iff every node and its label of level j are in one cluster of level j + 1 */
    for (int j = 0; j + 1 < n_levels; j++) {
        const int32_t *fine = labels + (size_t)j * (size_t)n, *coarse = fine + n;
        for (int32_t v = 0; v < n; v++)
            if (coarse[v] != coarse[fine[v]])
                return j + 1;
    }
    return 0;
}

int sat_cluster_reps(int n, const int32_t *label, const int32_t *degree, int32_t *rep, int32_t *size)
{
    if (n < 1 || !label || !rep || !size)
        return -1;
    for (int32_t v = 0; v < n; v++)
        if (label[v] < 0 || label[v] > v || label[label[v]] != label[v])
            return -1;
    /* first the roots' entries: a cluster's count and its best member so far, walking the nodes upwards (a later
     * member replaces the best only with a strictly larger degree) ... */
    int clusters = 0;
    for (int32_t v = 0; v < n; v++) {
        const int32_t l = label[v];
        if (l == v) {
            clusters++;
            size[v] = 1;
            rep[v] = v;
        } else {
            size[l]++;
            if (degree && degree[v] > degree[rep[l]])
                rep[l] = v;
        }
    }
    /* ... then every other member takes its root's (a root lies below its members and is final by now) */
    for (int32_t v = 0; v < n; v++)
        if (label[v] != v) {
            size[v] = size[label[v]];
            rep[v] = rep[label[v]];
        }
    return clusters;
}
