// Host build of the pose loss' shared math (tests/test_pose_loss_cpu.py): the fit fragment gdm_kabsch_fit.inc and the adjoint of
// gdm_pose_adjoint.h, included unchanged, around plain fp64 loops that restate steps 1, 4, 5 and 7 of THE POSE LOSS RULE.
// stdin: the number of cases; per case  n K S min_points cond_min up,  n rows  ax ay az bx by bz w,  12 numbers RT_gt,  K rows X,
// S x 12 numbers sym.  stdout: per case  state sym_idx loss  and n rows  dA (3) dw  as hexadecimal floats (every bit).
#include <math.h>
#include <stdio.h>
#include <vector>

#include "gdm_pose_adjoint.h"

static void fit(const double* st, double Rout[3][3], double cAo[3], double cBo[3], double So[3][3], float* o)
{
    const double n = st[0];
#include "gdm_kabsch_fit.inc"
    for (int i = 0; i < 3; ++i) {
        cAo[i] = cA[i]; cBo[i] = cB[i];
        for (int j = 0; j < 3; ++j) { Rout[i][j] = R[i][j]; So[i][j] = S[i][j]; }
    }
}

static void pose_error(const double R[3][3], const double t[3], const double* gt, const double* sym, const double* X, double* e)
{
    double q[3];
    for (int i = 0; i < 3; ++i) q[i] = ((sym[4 * i] * X[0] + sym[4 * i + 1] * X[1]) + sym[4 * i + 2] * X[2]) + sym[4 * i + 3];
    for (int i = 0; i < 3; ++i) {
        const double p = ((R[i][0] * X[0] + R[i][1] * X[1]) + R[i][2] * X[2]) + t[i];
        const double m = ((gt[4 * i] * q[0] + gt[4 * i + 1] * q[1]) + gt[4 * i + 2] * q[2]) + gt[4 * i + 3];
        e[i] = p - m;
    }
}

int main()
{
    int cases = 0;
    if (scanf("%d", &cases) != 1) return 2;
    for (int c = 0; c < cases; ++c) {
        int n, K, S, min_points;
        double cond_min, up;
        if (scanf("%d %d %d %d %lf %lf", &n, &K, &S, &min_points, &cond_min, &up) != 6 || n < 1 || K < 1 || S < 1) return 2;
        std::vector<double> P((size_t)n * 7), X((size_t)K * 3), sym((size_t)S * 12);
        double gt[12];
        for (double& v : P) if (scanf("%lf", &v) != 1) return 2;
        for (double& v : gt) if (scanf("%lf", &v) != 1) return 2;
        for (double& v : X) if (scanf("%lf", &v) != 1) return 2;
        for (double& v : sym) if (scanf("%lf", &v) != 1) return 2;

        double st[16] = {0};
        int count = 0;
        std::vector<char> usable(n);
        for (int i = 0; i < n; ++i) {
            const double* p = &P[(size_t)i * 7];
            const double w = p[6];
            usable[i] = (w > 0.0) && (w <= 1.79769313486231570e308);
            if (!usable[i]) continue;
            count += 1;
            st[0] += w;
            for (int a = 0; a < 3; ++a) {
                st[1 + a] += w * p[a];
                st[4 + a] += w * p[3 + a];
                for (int b = 0; b < 3; ++b) st[7 + 3 * a + b] += (w * p[a]) * p[3 + b];
            }
        }
        int state = 0, win = -1;
        double loss = 0.0, R[3][3], cA[3], cB[3], Sm[3][3], t[3], lam[3], V[3][3], Gamma[3][3] = {{0}}, Rtg[3] = {0}, g[3] = {0};
        float rt[12];
        if (count < min_points || !(st[0] > 0.0)) state = 1;
        else {
            fit(st, R, cA, cB, Sm, rt);
            for (int i = 0; i < 3; ++i) {
                t[i] = cB[i];
                for (int j = 0; j < 3; ++j) t[i] -= R[i][j] * cA[j];
            }
            state = gdm_pose_fit_condition(R, Sm, cond_min, lam, V);
        }
        if (state == 0) {
            double e[3], best = 0.0;
            for (int s = 0; s < S; ++s) {
                double sum = 0.0;
                for (int k = 0; k < K; ++k) {
                    pose_error(R, t, gt, &sym[(size_t)s * 12], &X[(size_t)k * 3], e);
                    sum += sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]);
                }
                const double D = sum / K;
                if (s == 0 || D < best) { best = D; win = s; }
            }
            loss = best;
            double G[3][3] = {{0}};
            for (int k = 0; k < K; ++k) {
                const double* x = &X[(size_t)k * 3];
                pose_error(R, t, gt, &sym[(size_t)win * 12], x, e);
                const double len = sqrt((e[0] * e[0] + e[1] * e[1]) + e[2] * e[2]);
                if (!(len > 0.0)) continue;
                for (int i = 0; i < 3; ++i) {
                    const double u = e[i] / len;
                    g[i] += u;
                    for (int j = 0; j < 3; ++j) G[i][j] += u * x[j];
                }
            }
            for (int i = 0; i < 3; ++i) {
                g[i] /= K;
                for (int j = 0; j < 3; ++j) G[i][j] /= K;
            }
            gdm_pose_fit_adjoint(R, cA, lam, V, G, g, Gamma, Rtg);
        }
        printf("%d %d %a\n", state, win, loss);
        for (int i = 0; i < n; ++i) {
            const double* p = &P[(size_t)i * 7];
            double dA[3] = {0, 0, 0}, dw = 0.0;
            if (state == 0 && usable[i]) {
                const double invW = 1.0 / st[0];
                double bg = 0.0;
                for (int a = 0; a < 3; ++a) {
                    const double bc[3] = {p[3] - cB[0], p[4] - cB[1], p[5] - cB[2]};
                    const double gb = (Gamma[a][0] * bc[0] + Gamma[a][1] * bc[1]) + Gamma[a][2] * bc[2];
                    const double da = gb - Rtg[a] * invW;
                    dA[a] = (p[6] * da) * up;
                    dw += (p[a] - cA[a]) * da;
                    bg += bc[a] * g[a];
                }
                dw = (dw + bg * invW) * up;
            }
            printf("%a %a %a %a\n", dA[0], dA[1], dA[2], dw);
        }
    }
    return 0;
}
