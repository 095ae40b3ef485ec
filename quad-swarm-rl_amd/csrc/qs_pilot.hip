// qs_pilot.hip - the device-side position controller behind include/quadswarm_control.h: the reference's NonlinearPositionController
// (gym_art/quadrotor_multi/quadrotor_control.py:282-330, numpy branch; Mellinger & Kumar 2011) for every drone of a handle in one launch,
// from the true state in the handle's wave-blocked state allocation.
//
// Mapping: one wave per state block, lane = the drone's lane of the step kernels (local env * N + drone), so a wave reads exactly the
// bytes of its block that the step kernel of the same block wrote - contiguous rows in the component-major order, 12 / 36 adjacent bytes per
// lane in the lane-major order - and writes 64 consecutive action rows; lanes behind the block's last drone (N does not divide 64, a
// partial last block) leave at once.  Per drone 21 state elements in (pos, vel, rot, omega, goal: 84 bytes in float32), 4 out, about 150
// flops: the launch is memory- and launch-bound.  Small batches run 64-thread workgroups - 8192 drones of 8-drone environments are 128
// waves, one per CU instead of four on each of 32 CUs - and large ones 256-thread workgroups (fewer workgroups to dispatch).
//
// Compiled without fast-math (native.UNIT_FLAGS): sqrt and the divisions are the correctly rounded ones.
#include "qs_pilot.h"   // with qs_state_blk.h: StateBlk, QS_BLK_AT, QS_WAVE - the block layout the controller reads the state from

#include <cmath>
#include <cstdlib>
#include <string>

template <typename real> struct PilotK {   // qs_pilot_params in the handle's precision, by value in the kernarg segment
    real kp_p, kd_p, kp_a, kd_a, yaw_gain, max_pos_err, gravity, x_des[3], jinv[4][4];
};

template <typename real> __device__ __forceinline__ real pilot_norm(const real *v) { return sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]); }
// quad_utils.py:80-86: below 1e-5 the vector is returned as it is
template <typename real> __device__ __forceinline__ void pilot_normalize(real *v) {
    const real n = pilot_norm(v);
    if (!(n < (real)0.00001)) { v[0] = v[0] / n; v[1] = v[1] / n; v[2] = v[2] / n; }
}
template <typename real> __device__ __forceinline__ void pilot_cross(const real *a, const real *b, real *o) {
    o[0] = a[1] * b[2] - a[2] * b[1]; o[1] = a[2] * b[0] - a[0] * b[2]; o[2] = a[0] * b[1] - a[1] * b[0];
}

typedef float pilot_f32x4 __attribute__((ext_vector_type(4)));
typedef double pilot_f64x2 __attribute__((ext_vector_type(2)));

// LM: the element order of the handle's blocks as a literal (StateBlk::lane_major), so that the accessor's order test folds away
template <typename real, int LM>
__device__ __forceinline__ void pilot_drone(StateBlk B, const PilotK<real> &k, int N, int e, int i, size_t g, real *out, const real *goals,
    int as_thrust) {
    B.lane_major = LM;
    real pos[3], vel[3], om[3], goal[3], R[9];
#pragma unroll
    for (int q = 0; q < 3; ++q) { pos[q] = QS_BLK_AT(real, B, pos, q, e, i, N); vel[q] = QS_BLK_AT(real, B, vel, q, e, i, N);
        om[q] = QS_BLK_AT(real, B, omega, q, e, i, N); }
#pragma unroll
    for (int q = 0; q < 9; ++q) R[q] = QS_BLK_AT(real, B, rot, q, e, i, N);   // row-major: R[3 * row + column]
    if (goals) { for (int q = 0; q < 3; ++q) goal[q] = goals[g * 3 + q]; }
    else { for (int q = 0; q < 3; ++q) goal[q] = QS_BLK_AT(real, B, goal, q, e, i, N); }

    real tg[3] = {goal[0] - pos[0], goal[1] - pos[1], goal[2] - pos[2]};
    const real dist = pilot_norm(tg);
    if (!(dist <= k.max_pos_err)) { const real s = k.max_pos_err / dist; tg[0] = s * tg[0]; tg[1] = s * tg[1]; tg[2] = s * tg[2]; }   // clamp_norm
    real acc[3] = {k.kp_p * tg[0] - k.kd_p * vel[0], k.kp_p * tg[1] - k.kd_p * vel[1], k.kp_p * tg[2] - k.kd_p * vel[2] + k.gravity};
    real zb[3] = {acc[0], acc[1], acc[2]}, yb[3], xb[3];
    pilot_normalize(zb);
    pilot_cross(zb, k.x_des, yb);
    pilot_normalize(yb);
    pilot_cross(yb, zb, xb);
    // A = R_des^T R with R_des = [xb yb zb] as columns: A[a][b] = (column a of R_des) . (column b of R); e_R = 1/2 vee(A - A^T)
#define QS_PILOT_DOT(v, col) (v[0] * R[col] + v[1] * R[3 + col] + v[2] * R[6 + col])
    real eR[3] = {(real)0.5 * (QS_PILOT_DOT(zb, 1) - QS_PILOT_DOT(yb, 2)), (real)0.5 * (QS_PILOT_DOT(xb, 2) - QS_PILOT_DOT(zb, 0)),
        (real)0.5 * (QS_PILOT_DOT(yb, 0) - QS_PILOT_DOT(xb, 1))};
    eR[2] *= k.yaw_gain;
    real des[4];
    des[0] = QS_PILOT_DOT(acc, 2);   // the acceleration wanted along the body's thrust axis
#undef QS_PILOT_DOT
#pragma unroll
    for (int q = 0; q < 3; ++q) des[1 + q] = -k.kp_a * eR[q] - k.kd_a * om[q];
    real t[4];
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        real x = k.jinv[m][0] * des[0] + k.jinv[m][1] * des[1] + k.jinv[m][2] * des[2] + k.jinv[m][3] * des[3];
        x = x < (real)0 ? (real)0 : (x > (real)1 ? (real)1 : x);
        t[m] = as_thrust ? x : (real)2 * x - (real)1;   // RawControl maps a back to 0.5 * (a + 1) (quadrotor_control.py:53-56)
    }
    if constexpr (sizeof(real) == 4) {
        const pilot_f32x4 v = {t[0], t[1], t[2], t[3]};
        *(pilot_f32x4 *)(out + g * 4) = v;
    } else {
        const pilot_f64x2 lo = {t[0], t[1]}, hi = {t[2], t[3]};
        *(pilot_f64x2 *)(out + g * 4) = lo; *(pilot_f64x2 *)(out + g * 4 + 2) = hi;
    }
}

template <typename real>
__global__ void __launch_bounds__(256) qs_pilot_kernel(const StateBlk B, const PilotK<real> k, int E, int N, real *out, const uint8_t *mask,
    const real *goals, int as_thrust) {
    const int blk = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    const int el = lane / N, i = lane - el * N, e = blk * (int)B.epb + el;
    if (el >= (int)B.epb || e >= E) return;          // idle lanes of a block, the blocks a rounded-up grid adds
    const size_t g = (size_t)e * N + i;
    if (mask && !mask[g]) return;                    // not this controller's drone: its action row is left alone
    if (B.lane_major) pilot_drone<real, 1>(B, k, N, e, i, g, out, goals, as_thrust);
    else pilot_drone<real, 0>(B, k, N, e, i, g, out, goals, as_thrust);
}

template <typename real> static void pilot_launch(const QsPilotView &v, const qs_pilot_params &p, void *out, const uint8_t *mask,
    const void *goals, int as_thrust, hipStream_t s) {
    PilotK<real> k;
    k.kp_p = (real)p.kp_p; k.kd_p = (real)p.kd_p; k.kp_a = (real)p.kp_a; k.kd_a = (real)p.kd_a; k.yaw_gain = (real)p.yaw_gain;
    k.max_pos_err = (real)p.max_pos_err; k.gravity = (real)p.gravity;
    for (int q = 0; q < 3; ++q) k.x_des[q] = (real)p.x_des[q];
    for (int a = 0; a < 4; ++a) for (int b = 0; b < 4; ++b) k.jinv[a][b] = (real)p.jinv[a][b];
    const int E = v.cfg->num_envs, N = v.cfg->num_agents, nblk = (E + (int)v.blk.epb - 1) / (int)v.blk.epb;
    const int waves = nblk <= 8 * v.cus ? 1 : 4;     // waves per workgroup: spread a small batch over the CUs
    hipLaunchKernelGGL(qs_pilot_kernel<real>, dim3((nblk + waves - 1) / waves), dim3(QS_WAVE * waves), 0, s, v.blk, k, E, N, (real *)out, mask,
        (const real *)goals, as_thrust);
}

extern "C" {

int qs_pilot_default_params(const qs_config *cfg, qs_pilot_params *out) {
    if (!cfg || !out) return qs_pilot_fail(QS_ERR_INVALID, "null argument");
    qs_pilot_params p = {};
    p.kp_p = 4.5; p.kd_p = 3.5; p.kp_a = 200.0; p.kd_a = 50.0; p.yaw_gain = 0.2; p.max_pos_err = 4.0;
    p.gravity = cfg->gravity;
    p.x_des[0] = 1.0;
    // quadrotor_jacobian (quadrotor_control.py:158-169): (acceleration along the thrust axis, angular acceleration) per unit of normalised thrust
    double a[4][8];
    for (int m = 0; m < 4; ++m) {
        a[0][m] = cfg->thrust_max[m] / cfg->mass;
        a[1][m] = cfg->thrust_max[m] * cfg->prop_cross[m][0] / cfg->inertia[0];
        a[2][m] = cfg->thrust_max[m] * cfg->prop_cross[m][1] / cfg->inertia[1];
        a[3][m] = cfg->torque_max[m] * cfg->prop_ccw[m] / cfg->inertia[2];
        for (int r = 0; r < 4; ++r) a[r][4 + m] = r == m ? 1.0 : 0.0;
    }
    for (int c = 0; c < 4; ++c) {   // Gauss-Jordan with partial pivoting on [J | I]
        int piv = c;
        for (int r = c + 1; r < 4; ++r) if (std::fabs(a[r][c]) > std::fabs(a[piv][c])) piv = r;
        if (!(std::fabs(a[piv][c]) > 0.0)) return qs_pilot_fail(QS_ERR_INVALID, "qs_pilot_default_params: the airframe's Jacobian is singular");
        for (int q = 0; q < 8; ++q) { const double t = a[c][q]; a[c][q] = a[piv][q]; a[piv][q] = t; }
        const double d = a[c][c];
        for (int q = 0; q < 8; ++q) a[c][q] /= d;
        for (int r = 0; r < 4; ++r) {
            if (r == c) continue;
            const double f = a[r][c];
            for (int q = 0; q < 8; ++q) a[r][q] -= f * a[c][q];
        }
    }
    for (int r = 0; r < 4; ++r) for (int q = 0; q < 4; ++q) p.jinv[r][q] = a[r][4 + q];
    *out = p;
    return QS_OK;
}

static int pilot_params_slot(const QsPilotView &v) {   // the handle's parameters, allocated on first use
    if (*v.params) return QS_OK;
    qs_pilot_params *p = (qs_pilot_params *)malloc(sizeof(qs_pilot_params));
    if (!p) return qs_pilot_fail(QS_ERR_INVALID, "out of host memory");
    const int rc = qs_pilot_default_params(v.cfg, p);
    if (rc != QS_OK) { free(p); return rc; }
    *v.params = p;
    return QS_OK;
}

int qs_pilot_set_params(qs_handle *h, const qs_pilot_params *p) {
    QsPilotView v;
    if (!p) return qs_pilot_fail(QS_ERR_INVALID, "null argument");
    if (int rc = qs_pilot_view(h, &v)) return rc;
    if (int rc = pilot_params_slot(v)) return rc;
    **v.params = *p;
    return QS_OK;
}

int qs_pilot_actions(qs_handle *h, void *actions_out_dev, const uint8_t *mask_dev, const void *goals_dev, int32_t as_thrust, void *stream) {
    QsPilotView v;
    if (int rc = qs_pilot_view(h, &v)) return rc;
    if (v.gate_resident) return qs_pilot_fail(QS_ERR_UNSUPPORTED,
        "qs_pilot_actions: a gated launch of this handle is resident and holds the state (qs_sync first)");
    void *out = actions_out_dev ? actions_out_dev : v.actions;
    if (((uintptr_t)out & 15) != 0) return qs_pilot_fail(QS_ERR_INVALID, "qs_pilot_actions: actions_out_dev must be 16-byte aligned");
    if (int rc = pilot_params_slot(v)) return rc;
    hipError_t e = hipSetDevice(v.device);
    if (e == hipSuccess) {
        if (v.real_size == 8) pilot_launch<double>(v, **v.params, out, mask_dev, goals_dev, as_thrust, (hipStream_t)stream);
        else pilot_launch<float>(v, **v.params, out, mask_dev, goals_dev, as_thrust, (hipStream_t)stream);
        e = hipGetLastError();
    }
    if (e != hipSuccess) return qs_pilot_fail(QS_ERR_HIP, (std::string("qs_pilot_actions: ") + hipGetErrorString(e)).c_str());
    return QS_OK;
}

}   // extern "C"
