/* Fit statistics of a global fit from plain C99 (vp_global_statistics): a double-exponential global fit (B = 2 problems of
 * S = 4 right-hand sides, weighted) with every output, the same call with the optional outputs NULL (bit-identical
 * Cov(alpha, alpha), chi^2, status), and on a single-RHS handle the blocks of vp_statistics' (n+q)^2 matrix.  Without a
 * GPU only the refusals run.  usage: test_global_statistics [expect_gpu] */
#include "varpro_hip.h"

#include <math.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#define M 512
#define S 4
#define B 2

static double rel(double a, double b) { return fabs(a - b) / (fabs(b) > 0 ? fabs(b) : 1.0); }

int main(int argc, char **argv) {
    const int expect_gpu = argc > 1 && strcmp(argv[1], "expect_gpu") == 0;
    int failures = 0, i, s, b, k, rc;
    vp_model_desc d;
    vp_batch *h = 0, *h1 = 0;
    static double t[M], w[M], y[B * S * M], y1[M], band[B * S * M], cc[B * S * 9], ca[B * S * 6];
    double alpha[B * 2] = {1.2, 3.5, 1.2, 3.5}, cov[B * 4], chi2[B], cov0[B * 4], chi20[B], a1[2] = {1.2, 3.5};
    double cov1[25], chi21, sig1[M], gcov1[4], gchi21, gcc1[9], gca1[6], gband1[M];
    int32_t st[B], st0[B], st1, gst1;
    vp_report rep[B];
    rc = vp_global_statistics(NULL, cov, chi2, NULL, NULL, NULL, st);
    if (rc != VP_ERR_INVALID) ++failures;
    memset(&d, 0, sizeof d);
    d.n_basis = 3;
    d.n_params = 2;
    d.kind[0] = VP_BASIS_EXP_DECAY; d.param[0][0] = 0; d.param[0][1] = -1;
    d.kind[1] = VP_BASIS_EXP_DECAY; d.param[1][0] = 1; d.param[1][1] = -1;
    d.kind[2] = VP_BASIS_CONST;     d.param[2][0] = -1; d.param[2][1] = -1;
    for (i = 0; i < M; ++i) {
        t[i] = 12.5 * i / (M - 1.0);
        w[i] = 0.5 + 1.5 * i / (M - 1.0);
    }
    for (b = 0; b < B; ++b)
        for (s = 0; s < S; ++s)
            for (i = 0; i < M; ++i) /* a deterministic "noise" of 1e-2 */
                y[(b * S + s) * M + i] = (1.0 + s) * exp(-t[i] / 1.0) + (2.0 + 0.5 * b) * exp(-t[i] / 3.0) + 0.5 * s +
                                         1e-2 * sin(12.9898 * (i + 1) * (s + 2) * (b + 3));
    rc = vp_batch_create(&h, &d, VP_F64, M, S, B, t, y, w, -1.0, VP_FLAG_OWN_STREAM, 0, NULL);
    if (rc != VP_ERR_OK) {
        printf("no device (%d: %s)\n", rc, vp_last_error());
        if (expect_gpu) ++failures;
        printf("%d failure(s)\n", failures);
        return failures ? 1 : 0;
    }
    rc = vp_global_statistics(h, cov, chi2, NULL, NULL, NULL, st); /* before any parameters */
    if (rc != VP_ERR_INVALID) ++failures;
    if (vp_fit(h, NULL, alpha, NULL, rep) != VP_ERR_OK || rep[0].termination <= 0 || rep[1].termination <= 0) ++failures;
    if (vp_global_statistics(h, cov, chi2, cc, ca, band, st) != VP_ERR_OK) ++failures;
    if (vp_global_statistics(h, cov0, chi20, NULL, NULL, NULL, st0) != VP_ERR_OK) ++failures;
    for (b = 0; b < B; ++b) {
        if (st[b] != 0 || st0[b] != 0 || !(chi2[b] > 0) || memcmp(&chi2[b], &chi20[b], sizeof(double))) ++failures;
        if (memcmp(&cov[b * 4], &cov0[b * 4], 4 * sizeof(double))) ++failures;
        if (!(cov[b * 4] > 0 && cov[b * 4 + 3] > 0) || rel(cov[b * 4 + 1], cov[b * 4 + 2]) > 1e-12) ++failures;
        for (k = 0; k < S * M; ++k)
            if (!(band[b * S * M + k] > 0)) {
                ++failures;
                break;
            }
        printf("problem %d: sd(tau) = (%.3e, %.3e), reduced chi2 %.4e\n", b, sqrt(cov[b * 4]), sqrt(cov[b * 4 + 3]), chi2[b]);
    }
    vp_batch_destroy(h);
    /* S = 1: the blocks of vp_statistics' matrix */
    memcpy(y1, y, sizeof y1);
    if (vp_batch_create(&h1, &d, VP_F64, M, 1, 1, t, y1, w, -1.0, VP_FLAG_OWN_STREAM, 0, NULL) != VP_ERR_OK) ++failures;
    if (vp_fit(h1, NULL, a1, NULL, rep) != VP_ERR_OK) ++failures;
    if (vp_statistics(h1, cov1, &chi21, sig1, &st1) != VP_ERR_OK) ++failures;
    if (vp_global_statistics(h1, gcov1, &gchi21, gcc1, gca1, gband1, &gst1) != VP_ERR_OK) ++failures;
    if (st1 != 0 || gst1 != 0 || rel(gchi21, chi21) > 1e-12) ++failures;
    for (i = 0; i < 2; ++i)
        for (k = 0; k < 2; ++k)
            if (rel(gcov1[i * 2 + k], cov1[(3 + i) * 5 + 3 + k]) > 1e-11) ++failures;
    for (i = 0; i < 3; ++i) {
        for (k = 0; k < 3; ++k)
            if (rel(gcc1[i * 3 + k], cov1[i * 5 + k]) > 1e-11) ++failures;
        for (k = 0; k < 2; ++k)
            if (rel(gca1[i * 2 + k], cov1[(3 + k) * 5 + i]) > 1e-11) ++failures;
    }
    for (i = 0; i < M; ++i)
        if (rel(gband1[i], sig1[i]) > 1e-11) {
            ++failures;
            break;
        }
    vp_batch_destroy(h1);
    printf("global statistics from C: %d failure(s)\n", failures);
    return failures ? 1 : 0;
}
