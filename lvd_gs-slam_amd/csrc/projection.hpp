// The projection arithmetic both per-Gaussian passes use (preprocess.hip: forward; preprocess_bwd.hip: backward): camera, 3-D and
// 2-D covariance, the EWA matrices, the SH basis and its gradient, the fused activations.  In an anonymous namespace: every
// translation unit that includes it has its own copy, inlined into its kernels.
#pragma once
#include "common.hpp"

namespace lvdgs {

namespace {

constexpr float SH_C0 = 0.28209479177387814f;
constexpr float SH_C1 = 0.4886025119029199f;
__device__ constexpr float SH_C2[5] = {1.0925484305920792f, -1.0925484305920792f, 0.31539156525252005f,
                                       -1.0925484305920792f, 0.5462742152960396f};
__device__ constexpr float SH_C3[7] = {-0.5900435899266435f, 2.890611442640554f, -0.4570457994644658f,
                                       0.3731763325901154f,  -0.4570457994644658f, 1.445305721320277f,
                                       -0.5900435899266435f};

struct Cam {
    const float *view, *proj, *proj_raw, *campos;
    float tanx, tany, fx, fy, scale_mod;
    int W, H, gx, gy, sh_degree, M;
};

__device__ __forceinline__ void xform3(const float p[3], const float *__restrict__ m, float o[3]) {
    o[0] = m[0] * p[0] + m[4] * p[1] + m[8] * p[2] + m[12];
    o[1] = m[1] * p[0] + m[5] * p[1] + m[9] * p[2] + m[13];
    o[2] = m[2] * p[0] + m[6] * p[1] + m[10] * p[2] + m[14];
}
__device__ __forceinline__ float xform_w(const float p[3], const float *__restrict__ m) {
    return m[3] * p[0] + m[7] * p[1] + m[11] * p[2] + m[15];
}

__device__ __forceinline__ void quat_rot(const float q[4], float R[3][3]) {
    const float r = q[0], x = q[1], y = q[2], z = q[3];
    R[0][0] = 1.f - 2.f * (y * y + z * z); R[0][1] = 2.f * (x * y - r * z); R[0][2] = 2.f * (x * z + r * y);
    R[1][0] = 2.f * (x * y + r * z); R[1][1] = 1.f - 2.f * (x * x + z * z); R[1][2] = 2.f * (y * z - r * x);
    R[2][0] = 2.f * (x * z - r * y); R[2][1] = 2.f * (y * z + r * x); R[2][2] = 1.f - 2.f * (x * x + y * y);
}

// Sigma = (R diag(mod*s)) (R diag(mod*s))^T as xx,xy,xz,yy,yz,zz
__device__ __forceinline__ void cov3d_of(const float s[3], float mod, const float q[4], float c6[6]) {
    float R[3][3], M[3][3];
    quat_rot(q, R);
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) M[i][j] = R[i][j] * (mod * s[j]);
    c6[0] = M[0][0] * M[0][0] + M[0][1] * M[0][1] + M[0][2] * M[0][2];
    c6[1] = M[0][0] * M[1][0] + M[0][1] * M[1][1] + M[0][2] * M[1][2];
    c6[2] = M[0][0] * M[2][0] + M[0][1] * M[2][1] + M[0][2] * M[2][2];
    c6[3] = M[1][0] * M[1][0] + M[1][1] * M[1][1] + M[1][2] * M[1][2];
    c6[4] = M[1][0] * M[2][0] + M[1][1] * M[2][1] + M[1][2] * M[2][2];
    c6[5] = M[2][0] * M[2][0] + M[2][1] * M[2][1] + M[2][2] * M[2][2];
}

struct Ewa {
    float T[2][3];
    float t[3];
    bool clx, cly;
};

__device__ __forceinline__ void ewa_setup(const float pv[3], const float *__restrict__ V, const Cam &c, Ewa &e) {
    const float limx = FOV_GUARD * c.tanx, limy = FOV_GUARD * c.tany;
    const float txtz = pv[0] / pv[2], tytz = pv[1] / pv[2];
    e.clx = (txtz < -limx) || (txtz > limx);
    e.cly = (tytz < -limy) || (tytz > limy);
    const float cx = txtz < -limx ? -limx : (txtz > limx ? limx : txtz);
    const float cy = tytz < -limy ? -limy : (tytz > limy ? limy : tytz);
    e.t[0] = cx * pv[2]; e.t[1] = cy * pv[2]; e.t[2] = pv[2];
    const float j00 = c.fx / e.t[2], j02 = -(c.fx * e.t[0]) / (e.t[2] * e.t[2]);
    const float j11 = c.fy / e.t[2], j12 = -(c.fy * e.t[1]) / (e.t[2] * e.t[2]);
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const float w0 = V[4 * k + 0], w1 = V[4 * k + 1], w2 = V[4 * k + 2];
        e.T[0][k] = j00 * w0 + j02 * w2;
        e.T[1][k] = j11 * w1 + j12 * w2;
    }
}

__device__ __forceinline__ void sym6(const float c6[6], float S[3][3]) {
    S[0][0] = c6[0]; S[0][1] = S[1][0] = c6[1]; S[0][2] = S[2][0] = c6[2];
    S[1][1] = c6[3]; S[1][2] = S[2][1] = c6[4]; S[2][2] = c6[5];
}

__device__ __forceinline__ void cov2d_of(const Ewa &e, const float c6[6], float &a, float &b, float &c) {
    float S[3][3], TS[2][3];
    sym6(c6, S);
#pragma unroll
    for (int i = 0; i < 2; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) TS[i][j] = e.T[i][0] * S[0][j] + e.T[i][1] * S[1][j] + e.T[i][2] * S[2][j];
    a = TS[0][0] * e.T[0][0] + TS[0][1] * e.T[0][1] + TS[0][2] * e.T[0][2] + LOWPASS;
    b = TS[0][0] * e.T[1][0] + TS[0][1] * e.T[1][1] + TS[0][2] * e.T[1][2];
    c = TS[1][0] * e.T[1][0] + TS[1][1] * e.T[1][1] + TS[1][2] * e.T[1][2] + LOWPASS;
}

__device__ __forceinline__ void sh_basis(int deg, const float d[3], float B[16]) {
    const float x = d[0], y = d[1], z = d[2];
#pragma unroll
    for (int k = 0; k < 16; k++) B[k] = 0.f;
    B[0] = SH_C0;
    if (deg > 0) {
        B[1] = -SH_C1 * y; B[2] = SH_C1 * z; B[3] = -SH_C1 * x;
        if (deg > 1) {
            const float xx = x * x, yy = y * y, zz = z * z, xy = x * y, yz = y * z, xz = x * z;
            B[4] = SH_C2[0] * xy; B[5] = SH_C2[1] * yz; B[6] = SH_C2[2] * (2.f * zz - xx - yy);
            B[7] = SH_C2[3] * xz; B[8] = SH_C2[4] * (xx - yy);
            if (deg > 2) {
                B[9] = SH_C3[0] * y * (3.f * xx - yy); B[10] = SH_C3[1] * xy * z;
                B[11] = SH_C3[2] * y * (4.f * zz - xx - yy); B[12] = SH_C3[3] * z * (2.f * zz - 3.f * xx - 3.f * yy);
                B[13] = SH_C3[4] * x * (4.f * zz - xx - yy); B[14] = SH_C3[5] * z * (xx - yy);
                B[15] = SH_C3[6] * x * (xx - 3.f * yy);
            }
        }
    }
}

// gradient of basis k w.r.t. the unit direction (x,y,z)
__device__ __forceinline__ void sh_basis_grad(int deg, const float d[3], float G[16][3]) {
    const float x = d[0], y = d[1], z = d[2];
#pragma unroll
    for (int k = 0; k < 16; k++) G[k][0] = G[k][1] = G[k][2] = 0.f;
    if (deg > 0) { G[1][1] = -SH_C1; G[2][2] = SH_C1; G[3][0] = -SH_C1; }
    if (deg > 1) {
        G[4][0] = SH_C2[0] * y; G[4][1] = SH_C2[0] * x;
        G[5][1] = SH_C2[1] * z; G[5][2] = SH_C2[1] * y;
        G[6][0] = SH_C2[2] * -2.f * x; G[6][1] = SH_C2[2] * -2.f * y; G[6][2] = SH_C2[2] * 4.f * z;
        G[7][0] = SH_C2[3] * z; G[7][2] = SH_C2[3] * x;
        G[8][0] = SH_C2[4] * 2.f * x; G[8][1] = SH_C2[4] * -2.f * y;
    }
    if (deg > 2) {
        const float xx = x * x, yy = y * y, zz = z * z;
        G[9][0] = SH_C3[0] * 6.f * x * y; G[9][1] = SH_C3[0] * (3.f * xx - 3.f * yy);
        G[10][0] = SH_C3[1] * y * z; G[10][1] = SH_C3[1] * x * z; G[10][2] = SH_C3[1] * x * y;
        G[11][0] = SH_C3[2] * -2.f * x * y; G[11][1] = SH_C3[2] * (4.f * zz - xx - 3.f * yy); G[11][2] = SH_C3[2] * 8.f * y * z;
        G[12][0] = SH_C3[3] * -6.f * x * z; G[12][1] = SH_C3[3] * -6.f * y * z; G[12][2] = SH_C3[3] * (6.f * zz - 3.f * xx - 3.f * yy);
        G[13][0] = SH_C3[4] * (4.f * zz - 3.f * xx - yy); G[13][1] = SH_C3[4] * -2.f * x * y; G[13][2] = SH_C3[4] * 8.f * x * z;
        G[14][0] = SH_C3[5] * 2.f * x * z; G[14][1] = SH_C3[5] * -2.f * y * z; G[14][2] = SH_C3[5] * (xx - yy);
        G[15][0] = SH_C3[6] * (3.f * xx - 3.f * yy); G[15][1] = SH_C3[6] * -6.f * x * y;
    }
}

// Optional activations fused into the projection (lvdgs_args.activations): the model's raw parameters are
// read and activated here, and preprocess_bwd applies the chain rule, instead of separate elementwise
// kernels (exp / sigmoid / normalise and their backward) before and after the rasterizer.
constexpr int ACT_EXP_SCALES = 1, ACT_NORMALIZE_ROT = 2, ACT_SIGMOID_OPACITY = 4;

// the activations of raw scales / rotations (s, q hold the raw values on entry)
__device__ __forceinline__ void activate_scale_rot(int act, float s[3], float q[4], float &qnorm) {
    if (act & ACT_EXP_SCALES) { s[0] = expf(s[0]); s[1] = expf(s[1]); s[2] = expf(s[2]); }
    qnorm = 1.f;
    if (act & ACT_NORMALIZE_ROT) {
        qnorm = fmaxf(sqrtf(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]), 1e-12f);
        q[0] /= qnorm; q[1] /= qnorm; q[2] /= qnorm; q[3] /= qnorm;
    }
}

Cam make_cam(const lvdgs_args &a) {
    Cam c;
    c.view = a.viewmatrix; c.proj = a.projmatrix; c.proj_raw = a.projmatrix_raw; c.campos = a.campos;
    c.tanx = a.tanfovx; c.tany = a.tanfovy;
    c.W = a.image_width; c.H = a.image_height;
    c.fx = (float)c.W / (2.0f * c.tanx); c.fy = (float)c.H / (2.0f * c.tany);
    c.scale_mod = a.scale_modifier;
    c.gx = (c.W + TILE - 1) / TILE; c.gy = (c.H + TILE - 1) / TILE;
    c.sh_degree = a.sh_degree; c.M = a.sh_coeffs;
    return c;
}

}  // namespace

}  // namespace lvdgs
