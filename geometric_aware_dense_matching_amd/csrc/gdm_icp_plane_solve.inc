// Statement fragment: the Gauss-Newton solve and pose update of one point-to-plane ICP iteration (include/gdm.h
// gdm_icp_plane_update_hip).  Included INSIDE a function body where these are in scope:
//   const double* ps     the 29 sums { A upper triangle, row-major (21), g (6), S = sum w, L2 = sum w |x|^2 }
//   const double* rt     the current pose [R | t], 12 values row-major (the kernel's fp32 pose, widened)
//   double        pivot_min
// It declares, for the code after it:
//   bool   degenerate    l2 <= 0 or a pivot of the scaled matrix below pivot_min; nothing below is meaningful then
//   double min_pivot     the smallest L_kk^2 reached (of the pivots computed)
//   double xi[6]         the increment (omega, v), A xi = -g
//   double Rn[3][3], tn[3]   the new pose R R_inc^T, t - Rn v in fp64 (the caller rounds them to fp32)
// A fragment rather than a __device__ function, as gdm_kabsch_fit.inc is, so that the same statements compile for the host.
//
// The degeneracy test is unit-free: with l2 = L2 / S (the weighted mean |x|^2) and D = diag(1/sqrt(l2) x3, 1 x3), the matrix
// D A D / S has entries of order 1 whatever the object's size or the number of pairs; it is factored by Cholesky in the given order,
// without pivoting.
    bool degenerate = false;
    double min_pivot = 1e300;
    double xi[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    double Rn[3][3], tn[3];
    for (int i = 0; i < 3; ++i) {
        tn[i] = rt[4 * i + 3];
        for (int j = 0; j < 3; ++j) Rn[i][j] = rt[4 * i + j];
    }
    {
        const double S = ps[27];
        const double l2 = ps[28] / S;
        if (!(l2 > 0.0)) degenerate = true;
        double L[6][6], y[6], sc = 0.0;
        if (!degenerate) {
            sc = 1.0 / sqrt(l2);
            int e = 0;
            for (int i = 0; i < 6; ++i)
                for (int j = i; j < 6; ++j) {
                    const double v = ps[e++] * (i < 3 ? sc : 1.0) * (j < 3 ? sc : 1.0) / S;
                    L[i][j] = v;                                         // the scaled matrix; the lower triangle becomes the factor
                    L[j][i] = v;
                }
            for (int i = 0; i < 6; ++i) y[i] = -ps[21 + i] * (i < 3 ? sc : 1.0) / S;
            for (int k = 0; k < 6 && !degenerate; ++k) {
                double p = L[k][k];
                for (int m = 0; m < k; ++m) p -= L[k][m] * L[k][m];
                if (p < min_pivot) min_pivot = p;
                if (!(p >= pivot_min)) { degenerate = true; break; }
                const double d = sqrt(p);
                L[k][k] = d;
                for (int i = k + 1; i < 6; ++i) {
                    double s = L[i][k];
                    for (int m = 0; m < k; ++m) s -= L[i][m] * L[k][m];
                    L[i][k] = s / d;
                }
            }
            if (!(min_pivot == min_pivot)) min_pivot = -1.0;             // NaN sums: degenerate, reported as a negative pivot
        }
        if (!degenerate) {
            for (int i = 0; i < 6; ++i) {                                // L z = y
                double s = y[i];
                for (int m = 0; m < i; ++m) s -= L[i][m] * y[m];
                y[i] = s / L[i][i];
            }
            for (int i = 5; i >= 0; --i) {                               // L^T u = z
                double s = y[i];
                for (int m = i + 1; m < 6; ++m) s -= L[m][i] * y[m];
                y[i] = s / L[i][i];
            }
            for (int i = 0; i < 6; ++i) xi[i] = y[i] * (i < 3 ? sc : 1.0);
            // R_inc = exp([omega]x) = I + a K + b K^2 (Rodrigues); first order below |omega| = 1e-8
            const double wx = xi[0], wy = xi[1], wz = xi[2];
            const double th = sqrt(wx * wx + wy * wy + wz * wz);
            double a = 1.0, b = 0.0;
            if (th >= 1e-8) { a = sin(th) / th; b = (1.0 - cos(th)) / (th * th); }
            const double K[3][3] = {{0.0, -wz, wy}, {wz, 0.0, -wx}, {-wy, wx, 0.0}};
            double Ri[3][3];
            for (int i = 0; i < 3; ++i)
                for (int j = 0; j < 3; ++j) {
                    double k2 = 0.0;
                    for (int m = 0; m < 3; ++m) k2 += K[i][m] * K[m][j];
                    Ri[i][j] = (i == j ? 1.0 : 0.0) + a * K[i][j] + b * k2;
                }
            double Rc[3][3];
            for (int i = 0; i < 3; ++i)
                for (int j = 0; j < 3; ++j) {                            // R R_inc^T
                    double s = 0.0;
                    for (int m = 0; m < 3; ++m) s += rt[4 * i + m] * Ri[j][m];
                    Rc[i][j] = s;
                }
            for (int i = 0; i < 3; ++i) {
                double s = rt[4 * i + 3];
                for (int j = 0; j < 3; ++j) { Rn[i][j] = Rc[i][j]; s -= Rc[i][j] * xi[3 + j]; }
                tn[i] = s;
            }
        }
    }
