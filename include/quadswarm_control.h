/*
 * quadswarm_control.h - C ABI of the device-side position controller: a third source of actions next to the caller's tensor and
 * the learned policy.  Exported by libquadswarm_hip.so; the handle and qs_config are those of quadswarm.h.
 *
 * What it computes is the reference's NonlinearPositionController (gym_art/quadrotor_multi/quadrotor_control.py:251-330, the
 * numpy branch `step`; "an 'oracle' policy to drive the quadrotor towards a goal", after Mellinger & Kumar 2011), for every drone
 * of a handle at once, from the TRUE state the stepper keeps in device memory - the reference reads dynamics.pos / vel / rot /
 * omega, not the noisy observation:
 *
 *     to_goal = clamp_norm(goal - pos, max_pos_err)                      (quad_utils.py:112-116)
 *     acc_des = kp_p * to_goal - kd_p * vel + (0, 0, gravity)
 *     zb = normalize(acc_des), yb = normalize(zb x x_des), xb = yb x zb   (normalize: the vector itself below a norm of 1e-5,
 *     R_des = [xb yb zb] (columns)                                         quad_utils.py:80-86)
 *     e_R = 1/2 vee(R_des^T R - R^T R_des), vee(M) = (M21, M02, M10);  e_R[2] *= yaw_gain
 *     dw_des = -kp_a * e_R - kd_a * omega
 *     thrusts = clip(jinv . (acc_des . R[:, 2], dw_des), 0, 1)
 *
 * One launch of its own (one lane per drone, about 150 flops and 100 bytes per drone in float32), stream-ordered and
 * allocation-free: it can be captured into a HIP graph between two qs_step launches.  The controller knows nothing of
 * neighbours or obstacles.  The TensorFlow branch of the reference class and raw_control=False are out of scope.
 */
#ifndef QUADSWARM_CONTROL_H
#define QUADSWARM_CONTROL_H

#include <stdint.h>

#include "quadswarm.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct qs_pilot_params {
    double kp_p, kd_p, kp_a, kd_a;   /* 4.5 3.5 200 50 (quadrotor_control.py:266-267) */
    double yaw_gain, max_pos_err;    /* 0.2, 4.0 (:315, :287) */
    double gravity;                  /* cfg.gravity */
    double x_des[3];                 /* rot_des[:, 0] = (1, 0, 0) (:269, :300) */
    double jinv[4][4];               /* inverse of quadrotor_jacobian (:158-169) */
} qs_pilot_params;

/* The reference's gains and the inverse Jacobian of the airframe in `cfg` (host only, touches no GPU).  Jacobian rows: thrust_max / mass;
 * thrust_max[m] * prop_cross[m][0 | 1] / inertia[0 | 1]; torque_max[m] * prop_ccw[m] / inertia[2].  Inverted in double.
 * QS_ERR_INVALID for a null argument or a singular Jacobian. */
int qs_pilot_default_params(const qs_config *cfg, qs_pilot_params *out);

/* Replace the parameters the handle's following qs_pilot_actions launches use (optional: qs_pilot_default_params of the handle's
 * configuration otherwise).  The values travel in launch arguments: a captured graph keeps the ones it was recorded with. */
int qs_pilot_set_params(qs_handle *h, const qs_pilot_params *p);

/* Controller output of every drone of the handle, as ONE launch on `stream`:
 *   actions_out_dev  real [E*N, 4] row-major, device, 16-byte aligned, of the handle's precision; NULL = qs_buffers.actions (what
 *                    qs_step(h, NULL, stream) consumes)
 *   mask_dev         NULL, or uint8 [E*N], device: rows whose byte is 0 are NOT WRITTEN - whatever the caller put there (a policy's
 *                    actions) stays bit for bit
 *   goals_dev        NULL, or real [E*N, 3] row-major, device: these goals instead of the state's (scripted waypoints)
 *   as_thrust        0: the raw action a = 2 t - 1 that RawControl maps back to the thrusts t (quadrotor_control.py:53-56);
 *                    otherwise the thrusts t themselves
 * QS_ERR_UNSUPPORTED while a gated launch of the handle is resident (qs_step_gated: the state is not in device memory then; qs_sync
 * ends that). */
int qs_pilot_actions(qs_handle *h, void *actions_out_dev, const uint8_t *mask_dev, const void *goals_dev, int32_t as_thrust, void *stream);

#ifdef __cplusplus
}
#endif

/* The stepper's other add-on with launches of its own next to the step kernel, the episode summary, has a header of its own; it is part of
 * this one so that a caller of the add-ons has one header to include (either may come first: both only need quadswarm.h). */
#include "quadswarm_summary.h"
/* ... and so do the neighbour identities of the observation rows */
#include "quadswarm_neighbors.h"
#endif
