/*
 * fks_rotation_mean.h — the pieces of a rotation mean (Markley's: the dominant eigenvector of the
 * sum of q q^T), shared by the summary kernels (fks_kernels.hip) and their host twin
 * (fks_summary.cpp), so both evaluate the same expression trees: the quaternion of a rotation
 * block by Shepperd's largest-component rule, the cyclic Jacobi iteration on a symmetric 4 x 4
 * matrix, and the rotation of a quaternion.  Only + - * / and sqrt; the statement is in
 * fks_capi.h (fks_summarize_clusters).
 */
#ifndef FKS_ROTATION_MEAN_H
#define FKS_ROTATION_MEAN_H

#include "fks_portable_math.h"

namespace fks_rotmean {

using fks_math::dabs;
using fks_math::dsqrt;

constexpr int kProducts = 10;        /* q_a q_b for a <= b, row-major over the upper triangle */
constexpr int kMaxSweeps = 16;       /* the sweep cap */
constexpr double kNegligible = 0x1p-80; /* an off-diagonal at or below this times the trace is set to zero */

/* q = (w, x, y, z) of the rotation block of T (3 x 4 row-major): the largest of (trace, R00, R11,
 * R22) chooses the component taken from the square root, the lowest index winning a tie */
FKS_HD inline void quat_of_rotation34(const double* T, double* q) {
    const double R00 = T[0], R01 = T[1], R02 = T[2], R10 = T[4], R11 = T[5], R12 = T[6], R20 = T[8], R21 = T[9], R22 = T[10];
    const double tr = (R00 + R11) + R22;
    int k = 0;
    double best = tr;
    if (R00 > best) {
        best = R00;
        k = 1;
    }
    if (R11 > best) {
        best = R11;
        k = 2;
    }
    if (R22 > best) k = 3;
    if (k == 0) {
        const double w = 0.5 * dsqrt(1.0 + tr);
        const double f = 0.25 / w;
        q[0] = w;
        q[1] = (R21 - R12) * f;
        q[2] = (R02 - R20) * f;
        q[3] = (R10 - R01) * f;
    } else if (k == 1) {
        const double x = 0.5 * dsqrt(((1.0 + R00) - R11) - R22);
        const double f = 0.25 / x;
        q[0] = (R21 - R12) * f;
        q[1] = x;
        q[2] = (R01 + R10) * f;
        q[3] = (R02 + R20) * f;
    } else if (k == 2) {
        const double y = 0.5 * dsqrt(((1.0 + R11) - R00) - R22);
        const double f = 0.25 / y;
        q[0] = (R02 - R20) * f;
        q[1] = (R01 + R10) * f;
        q[2] = y;
        q[3] = (R12 + R21) * f;
    } else {
        const double z = 0.5 * dsqrt(((1.0 + R22) - R00) - R11);
        const double f = 0.25 / z;
        q[0] = (R10 - R01) * f;
        q[1] = (R02 + R20) * f;
        q[2] = (R12 + R21) * f;
        q[3] = z;
    }
}

/* the ten products of q, in the order (0,0)(0,1)(0,2)(0,3)(1,1)(1,2)(1,3)(2,2)(2,3)(3,3) */
FKS_HD inline void quat_products(const double* q, double* p) {
    int k = 0;
    for (int a = 0; a < 4; ++a)
        for (int b = a; b < 4; ++b) p[k++] = q[a] * q[b];
}

/* The unit eigenvector of the largest eigenvalue of the symmetric 4 x 4 matrix whose upper
 * triangle is s[10] (the order of quat_products), by the cyclic Jacobi iteration of fks_capi.h.
 * max_sweeps is kMaxSweeps everywhere but in a test of the sweep cap. */
FKS_HD inline void dominant_eigenvector4(const double* s, double* v, int max_sweeps = kMaxSweeps) {
    double A[4][4], V[4][4];
    {
        int k = 0;
        for (int a = 0; a < 4; ++a)
            for (int b = a; b < 4; ++b) {
                A[a][b] = s[k];
                A[b][a] = s[k];
                ++k;
            }
    }
    for (int a = 0; a < 4; ++a)
        for (int b = 0; b < 4; ++b) V[a][b] = (a == b) ? 1.0 : 0.0;
    const double small = kNegligible * ((A[0][0] + A[1][1]) + (A[2][2] + A[3][3]));
    for (int sweep = 0; sweep < max_sweeps; ++sweep) {
        bool clean = true;
        for (int p = 0; p < 3; ++p)
            for (int q = p + 1; q < 4; ++q) {
                const double apq = A[p][q];
                if (apq == 0.0) continue;
                if (dabs(apq) <= small) {
                    A[p][q] = 0.0;
                    A[q][p] = 0.0;
                    continue;
                }
                clean = false;
                const double theta = (A[q][q] - A[p][p]) / (2.0 * apq);
                const double r = dabs(theta) + dsqrt(theta * theta + 1.0);
                const double t = (theta < 0.0) ? -1.0 / r : 1.0 / r;
                const double c = 1.0 / dsqrt(t * t + 1.0);
                const double sn = t * c;
                A[p][p] = A[p][p] - t * apq;
                A[q][q] = A[q][q] + t * apq;
                A[p][q] = 0.0;
                A[q][p] = 0.0;
                for (int r2 = 0; r2 < 4; ++r2) {
                    if (r2 != p && r2 != q) {
                        const double arp = A[r2][p], arq = A[r2][q];
                        const double np = c * arp - sn * arq;
                        const double nq = sn * arp + c * arq;
                        A[r2][p] = np;
                        A[p][r2] = np;
                        A[r2][q] = nq;
                        A[q][r2] = nq;
                    }
                    const double vrp = V[r2][p], vrq = V[r2][q];
                    V[r2][p] = c * vrp - sn * vrq;
                    V[r2][q] = sn * vrp + c * vrq;
                }
            }
        if (clean) break;
    }
    int k = 0;
    for (int a = 1; a < 4; ++a)
        if (A[a][a] > A[k][k]) k = a;
    /* the branches keep V in registers: no dynamically indexed column */
    double e0 = V[0][0], e1 = V[1][0], e2 = V[2][0], e3 = V[3][0];
    for (int a = 1; a < 4; ++a)
        if (k == a) {
            e0 = V[0][a];
            e1 = V[1][a];
            e2 = V[2][a];
            e3 = V[3][a];
        }
    const double nrm = dsqrt((e0 * e0 + e1 * e1) + (e2 * e2 + e3 * e3));
    v[0] = e0 / nrm;
    v[1] = e1 / nrm;
    v[2] = e2 / nrm;
    v[3] = e3 / nrm;
}

/* the rotation block of q = (w, x, y, z) into T (3 x 4 row-major; the translation column is left):
 * every entry is built from products of two components, so q and -q give the same bits */
FKS_HD inline void rotation34_of_quat(const double* q, double* T) {
    const double w = q[0], x = q[1], y = q[2], z = q[3];
    const double xx = x * x, yy = y * y, zz = z * z;
    const double xy = x * y, xz = x * z, yz = y * z, wx = w * x, wy = w * y, wz = w * z;
    T[0] = 1.0 - 2.0 * (yy + zz);
    T[1] = 2.0 * (xy - wz);
    T[2] = 2.0 * (xz + wy);
    T[4] = 2.0 * (xy + wz);
    T[5] = 1.0 - 2.0 * (xx + zz);
    T[6] = 2.0 * (yz - wx);
    T[8] = 2.0 * (xz - wy);
    T[9] = 2.0 * (yz + wx);
    T[10] = 1.0 - 2.0 * (xx + yy);
}

}  // namespace fks_rotmean

#endif
