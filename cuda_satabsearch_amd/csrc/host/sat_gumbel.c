/* sat_gumbel.c - see sat_gumbel.h */
#include <math.h>
#include <stddef.h>
#include "sat_gumbel.h"

static const double k_euler_gamma = 0.5772156649015328606;

static double pi_over_sqrt6(void)
{
    return M_PI / sqrt(6.0);
}

double sat_norm2(int score, int n1, int n2)
{
    return 2.0 * score / ((double)(n1 + n2));
}

double sat_z_gumbel_trunc(double norm2score)
{
    int x = (int)norm2score; /* the reference's implicit double -> int */
    double mu = SAT_GUMBEL_A + SAT_GUMBEL_B * k_euler_gamma;
    double sigma = pi_over_sqrt6() * SAT_GUMBEL_B;
    return (x - mu) / sigma;
}

double sat_pv_gumbel(double z)
{
    return 1 - exp(-exp(-(pi_over_sqrt6() * z + k_euler_gamma)));
}

/* ---- fitted statistics (sat_gumbel.h) */

int sat_stat_bin(int score, int n1, int n2)
{
    return score < 0 ? -1 : sat_stat_bin_of(score, n1 + n2);
}

void sat_stat_histogram(const int32_t *scores, int n, int n1, const int32_t *orders, uint32_t *counts, int32_t *below)
{
    for (int e = 0; e < n; e++) {
        if (scores[e] < 0) ++*below;
        else counts[sat_stat_bin_of(scores[e], n1 + orders[e])]++;
    }
}

void sat_gumbel_fit_table(double a, double b, double *z, double *p)
{
    const double mu = a + b * k_euler_gamma;
    const double sigma = pi_over_sqrt6() * b;
    for (int k = 0; k < SAT_STAT_BINS; k++) {
        z[k] = (k / (double)SAT_STAT_BINS_PER_UNIT - mu) / sigma;
        p[k] = sat_pv_gumbel(z[k]);
    }
}

/* the censored log-likelihood of bins 0 .. hi (and n_c rows above x_c) at (a, beta = log b), its gradient g[2] and
 * Hessian h[3] = {aa, a beta, beta beta} */
static double fit_eval(const uint32_t *counts, int hi, double n_c, double x_c, double a, double beta, double g[2], double h[3])
{
    const double b = exp(beta);
    double l = 0.0;
    g[0] = g[1] = h[0] = h[1] = h[2] = 0.0;
    for (int k = 0; k <= hi; k++) {
        if (!counts[k]) continue;
        const double c = (double)counts[k];
        const double t = ((k + 0.5) / SAT_STAT_BINS_PER_UNIT - a) / b;
        const double e = exp(-t);
        const double f1 = e - 1.0, f2 = -e;              /* f = -t - exp(-t): f', f'' */
        l += c * (-beta - t - e);
        g[0] += c * (-f1 / b);
        g[1] += c * (-1.0 - f1 * t);
        h[0] += c * (f2 / (b * b));
        h[1] += c * ((f2 * t + f1) / b);
        h[2] += c * (f2 * t * t + f1 * t);
    }
    if (n_c > 0.0) {
        /* g(t) = log(1 - exp(-u)), u = exp(-t): g' = -u / expm1(u), g'' = u * d/du (u / expm1(u)) */
        const double t = (x_c - a) / b;
        const double u = exp(-t);
        const double em = expm1(u);
        const double g1 = u > 0.0 ? -u / em : -1.0;
        double dh;                                       /* d/du (u / expm1(u)) */
        if (u < 1e-4) dh = -0.5 + u / 6.0;
        else dh = (em - u * (em + 1.0)) / (em * em);
        const double g2 = u * dh;
        l += n_c * (u > 0.0 ? log(-expm1(-u)) : -t);
        g[0] += n_c * (-g1 / b);
        g[1] += n_c * (-g1 * t);
        h[0] += n_c * (g2 / (b * b));
        h[1] += n_c * ((g2 * t + g1) / b);
        h[2] += n_c * (g2 * t * t + g1 * t);
    }
    return l;
}

int sat_gumbel_fit_binned(const uint32_t *counts, double censor, sat_fit *out)
{
    if (!counts || !out || !(censor >= 0.0 && censor <= 0.5)) return SAT_EINVAL;
    long long n = 0;
    for (int k = 0; k < SAT_STAT_BINS; k++) n += counts[k];
    out->a = SAT_GUMBEL_A;
    out->b = SAT_GUMBEL_B;
    out->rows = (int32_t)n;
    out->censored = 0;
    out->below = 0;
    out->fitted = 0;
    /* censoring: the overflow bin, then whole bins from the top */
    long long n_c = counts[SAT_STAT_BINS - 1];
    long long limit = (long long)floor(censor * (double)n);
    if (limit < n_c) limit = n_c;
    int hi = SAT_STAT_BINS - 2;
    while (hi >= 0 && n_c + (long long)counts[hi] <= limit) n_c += counts[hi--];
    out->censored = (int32_t)n_c;
    const double x_c = (hi + 1) / (double)SAT_STAT_BINS_PER_UNIT;
    /* the start: moments of the uncensored bins */
    int occupied = 0;
    double m = 0.0, v = 0.0, nu = 0.0;
    for (int k = 0; k <= hi; k++)
        if (counts[k]) {
            occupied++;
            nu += counts[k];
            m += counts[k] * ((k + 0.5) / SAT_STAT_BINS_PER_UNIT);
        }
    if (occupied < 2) return 0;
    m /= nu;
    for (int k = 0; k <= hi; k++) {
        const double d = (k + 0.5) / SAT_STAT_BINS_PER_UNIT - m;
        v += counts[k] * d * d;
    }
    v /= nu;
    double b0 = sqrt(6.0 * v) / M_PI;
    double a = m - k_euler_gamma * b0, beta = log(b0);
    double g[2], h[3];
    double l = fit_eval(counts, hi, (double)n_c, x_c, a, beta, g, h);
    const double tol = 1e-12 * (double)n;
    int converged = 0;
    for (int iter = 0; iter < 200 && isfinite(l); iter++) {
        if (fabs(g[0]) <= tol && fabs(g[1]) <= tol) { converged = 1; break; }
        /* Newton step on (a, beta); where the Hessian is not negative definite it is shifted until it is */
        double shift = 0.0, da = 0.0, db = 0.0;
        for (int tries = 0; tries < 60; tries++) {
            const double haa = h[0] - shift, hbb = h[2] - shift, det = haa * hbb - h[1] * h[1];
            if (haa < 0.0 && det > 0.0) {
                da = -(hbb * g[0] - h[1] * g[1]) / det;
                db = -(haa * g[1] - h[1] * g[0]) / det;
                break;
            }
            shift = shift > 0.0 ? 4.0 * shift : 1e-3 * (fabs(h[0]) + fabs(h[2]) + 1.0);
        }
        if (da == 0.0 && db == 0.0) break;
        /* step halving: never go downhill (up to the rounding of the sum) */
        int moved = 0;
        double step = 1.0;
        for (int halve = 0; halve < 50; halve++, step *= 0.5) {
            double g2[2], h2[3];
            const double l2 = fit_eval(counts, hi, (double)n_c, x_c, a + step * da, beta + step * db, g2, h2);
            if (isfinite(l2) && l2 >= l - 1e-14 * fabs(l)) {
                a += step * da;
                beta += step * db;
                l = l2;
                g[0] = g2[0]; g[1] = g2[1];
                h[0] = h2[0]; h[1] = h2[1]; h[2] = h2[2];
                moved = 1;
                break;
            }
        }
        if (!moved) break;
    }
    /* a stalled iteration still counts when the score equations hold to 1e-10 of the rows */
    if (!converged && isfinite(l) && fabs(g[0]) <= 1e-10 * (double)n && fabs(g[1]) <= 1e-10 * (double)n) converged = 1;
    const double b = exp(beta);
    if (!converged || !isfinite(a) || !isfinite(b) || !(b > 0.0)) return 0;
    out->a = a;
    out->b = b;
    out->fitted = 1;
    return 0;
}
