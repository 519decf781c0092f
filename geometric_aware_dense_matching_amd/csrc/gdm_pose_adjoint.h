// Steps 3 and 6 of THE POSE LOSS RULE (include/gdm.h): the conditioning of a weighted Kabsch fit and the adjoint of the fit, in fp64.
// Plain inline functions with nothing of the device in them, as gdm_kabsch_fit.inc has nothing: the kernels of gdm_poseloss.hip call
// them on one lane, and a g++ host build includes this file unchanged (tests/pose_adjoint_host.cpp) to be held against fp64 autograd.
//
// The fit maximises tr(R S), S = sum w (A - cA)(B - cB)^T, so R S is symmetric at the optimum and P = sym(R S) carries the
// singular values of S (the smallest with the sign of det) as its eigenvalues.  A rotation of the fit by a small antisymmetric
// Omega' (R -> (I + Omega') R) answers a change dS by  Omega' P + P Omega' = -(R dS - dS^T R^T);  that operator is self-adjoint on
// antisymmetric matrices, which gives dL/dS = -2 R^T Omega with Omega P + P Omega = skew(G' R^T) -- one 3x3 solve, no SVD derivative.
#pragma once
#ifdef __HIPCC__
#define GDM_POSE_ADJ_FN __host__ __device__ static inline
#else
#include <math.h>
#define GDM_POSE_ADJ_FN static inline
#endif

// Eigenvalues lam[3] (in no order) and eigenvectors (the columns of V) of the symmetric 3x3 P, by cyclic Jacobi as the fit's 4x4.
GDM_POSE_ADJ_FN void gdm_sym3_eig(const double P[3][3], double lam[3], double V[3][3])
{
    double A[3][3];
    double scale = 0.0;
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) { A[i][j] = P[i][j]; V[i][j] = (i == j) ? 1.0 : 0.0; scale = fmax(scale, fabs(P[i][j])); }
    for (int sweep = 0; sweep < 16; ++sweep) {
        double off = 0.0;
        for (int p = 0; p < 2; ++p)
            for (int q = p + 1; q < 3; ++q) off = fmax(off, fabs(A[p][q]));
        if (off <= 1e-18 * scale) break;
        for (int p = 0; p < 2; ++p)
            for (int q = p + 1; q < 3; ++q) {
                const double apq = A[p][q];
                if (fabs(apq) <= 1e-300) continue;
                const double theta = (A[q][q] - A[p][p]) / (2.0 * apq);
                const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
                for (int k = 0; k < 3; ++k) {                            // A <- A J
                    const double akp = A[k][p], akq = A[k][q];
                    A[k][p] = c * akp - s * akq; A[k][q] = s * akp + c * akq;
                }
                for (int k = 0; k < 3; ++k) {                            // A <- J^T A
                    const double apk = A[p][k], aqk = A[q][k];
                    A[p][k] = c * apk - s * aqk; A[q][k] = s * apk + c * aqk;
                }
                for (int k = 0; k < 3; ++k) {
                    const double vkp = V[k][p], vkq = V[k][q];
                    V[k][p] = c * vkp - s * vkq; V[k][q] = s * vkp + c * vkq;
                }
            }
    }
    for (int i = 0; i < 3; ++i) lam[i] = A[i][i];
}

// Step 3: P = (R S + (R S)^T) / 2 with its eigen-decomposition; 2 (ill-conditioned) when, with l1 >= l2 >= l3 its eigenvalues,
// l2 + l3 <= cond_min l1 (a NaN anywhere fails the comparison and is ill-conditioned too), else 0.
GDM_POSE_ADJ_FN int gdm_pose_fit_condition(const double R[3][3], const double S[3][3], double cond_min, double lam[3], double V[3][3])
{
    double M[3][3], P[3][3];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) M[i][j] = (R[i][0] * S[0][j] + R[i][1] * S[1][j]) + R[i][2] * S[2][j];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) P[i][j] = 0.5 * (M[i][j] + M[j][i]);
    gdm_sym3_eig(P, lam, V);
    double l1 = fmax(lam[0], fmax(lam[1], lam[2])), l3 = fmin(lam[0], fmin(lam[1], lam[2]));
    const double l2 = ((lam[0] + lam[1]) + lam[2]) - l1 - l3;
    return ((l2 + l3) > cond_min * l1) ? 0 : 2;
}

// Step 6: from the upstream G = dL/dR and g = dL/dt of a fitted crop (state 0; lam, V from gdm_pose_fit_condition) to
// Gamma = dL/dS = -2 R^T Omega and Rtg = R^T g  (dL/dcA = -Rtg, dL/dcB = g).
GDM_POSE_ADJ_FN void gdm_pose_fit_adjoint(const double R[3][3], const double cA[3], const double lam[3], const double V[3][3],
                                          const double G[3][3], const double g[3], double Gamma[3][3], double Rtg[3])
{
    double Gp[3][3], Z[3][3];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) Gp[i][j] = G[i][j] - g[i] * cA[j];
    for (int i = 0; i < 3; ++i)
        for (int j = 0; j < 3; ++j) Z[i][j] = (Gp[i][0] * R[j][0] + Gp[i][1] * R[j][1]) + Gp[i][2] * R[j][2];
    // axial(Za), Za = (Z - Z^T) / 2:  Za x = z cross x
    const double z[3] = {0.5 * (Z[2][1] - Z[1][2]), 0.5 * (Z[0][2] - Z[2][0]), 0.5 * (Z[1][0] - Z[0][1])};
    // (tr(P) I - P) omega = z in the eigenbasis of P: the eigenvalues of that matrix are the sums of two of P's
    const double tr = (lam[0] + lam[1]) + lam[2];
    double om[3] = {0.0, 0.0, 0.0};
    for (int k = 0; k < 3; ++k) {
        const double c = ((V[0][k] * z[0] + V[1][k] * z[1]) + V[2][k] * z[2]) / (tr - lam[k]);
        for (int i = 0; i < 3; ++i) om[i] += V[i][k] * c;
    }
    const double Om[3][3] = {{0.0, -om[2], om[1]}, {om[2], 0.0, -om[0]}, {-om[1], om[0], 0.0}};
    for (int i = 0; i < 3; ++i) {
        for (int j = 0; j < 3; ++j) Gamma[i][j] = -2.0 * ((R[0][i] * Om[0][j] + R[1][i] * Om[1][j]) + R[2][i] * Om[2][j]);
        Rtg[i] = (R[0][i] * g[0] + R[1][i] * g[1]) + R[2][i] * g[2];
    }
}
