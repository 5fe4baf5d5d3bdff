// gr_diff.h — one env's step of the differentiable window (gr_diff.hip): the lean forward arithmetic restated
// (action_scale, ctbr_compute<NO_MOTOR>, dd_explicit of gr_kernels.hip: the same expressions in the same order, built
// with -ffp-contract=off, pinned bit for bit by tests/test_gpu_diff_record.py), the three loss terms and the step's
// adjoint.  Plain float arrays, host + device, so the arithmetic can also be compiled and checked on a CPU.
//
// Reference: CTBRController.compute (extensions/diff.lab/diff/lab/controllers/controller_diff.py:120-138),
// DroneDynamics.step / align (.../quadcopter_diff/mdp/dynamics/droneDynamics.py:119-135, 156-180), the racing losses
// (.../quadcopter_diff/mdp/losses.py:72-117).
#pragma once
#include "gr_math.h"

// what the kernels need of the context, by value (one kernarg fetch)
struct gr_diff_consts {
  int num_envs, lag, dr_plant, num_levels;
  int max_gates, num_types, pad1, pad2;
  float dt, gravity, thrust_ratio, rate_bound;
  float thrust_lo, thrust_hi, gamma, pad3;
  float inertia[3];  // nominal (the controller's)
  float w_target;
  float w_vel, w_fall, pad4, pad5;
};

// one env's pre-step fields of a step (tape planes GR_DT_POSQ .. GR_DT_PAR3)
struct gr_diff_env {
  float p[3], q[4], v[3], w[3], al[3], T, tau[3], u[4];
  float thr, k2[3], k1[3], Kp[3], cT, Kd[3], mp, ct[3], mc, J[3];
};

GR_HD void gr_diff_cross3(const float a[3], const float b[3], float o[3]) {
  o[0] = a[1] * b[2] - a[2] * b[1];
  o[1] = a[2] * b[0] - a[0] * b[2];
  o[2] = a[0] * b[1] - a[1] * b[0];
}
GR_HD float gr_diff_dot3(const float a[3], const float b[3]) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }
// Isaac Lab quat_rotate / quat_rotate_inverse / quat_mul, as gr_kernels.hip states them
GR_HD void gr_diff_quat_rotate(const float q[4], const float v[3], float o[3]) {
  float s = 2.0f * (q[0] * q[0]) - 1.0f;
  float cx = q[2] * v[2] - q[3] * v[1];
  float cy = q[3] * v[0] - q[1] * v[2];
  float cz = q[1] * v[1] - q[2] * v[0];
  float d = (q[1] * v[0] + q[2] * v[1]) + q[3] * v[2];
  o[0] = (v[0] * s + (cx * q[0]) * 2.0f) + (q[1] * d) * 2.0f;
  o[1] = (v[1] * s + (cy * q[0]) * 2.0f) + (q[2] * d) * 2.0f;
  o[2] = (v[2] * s + (cz * q[0]) * 2.0f) + (q[3] * d) * 2.0f;
}
GR_HD void gr_diff_quat_rotate_inverse(const float q[4], const float v[3], float o[3]) {
  float s = 2.0f * (q[0] * q[0]) - 1.0f;
  float cx = q[2] * v[2] - q[3] * v[1];
  float cy = q[3] * v[0] - q[1] * v[2];
  float cz = q[1] * v[1] - q[2] * v[0];
  float d = (q[1] * v[0] + q[2] * v[1]) + q[3] * v[2];
  o[0] = (v[0] * s - (cx * q[0]) * 2.0f) + (q[1] * d) * 2.0f;
  o[1] = (v[1] * s - (cy * q[0]) * 2.0f) + (q[2] * d) * 2.0f;
  o[2] = (v[2] * s - (cz * q[0]) * 2.0f) + (q[3] * d) * 2.0f;
}
GR_HD void gr_diff_quat_mul(const float a[4], const float b[4], float o[4]) {
  float ww = (a[3] + a[1]) * (b[1] + b[2]);
  float yy = (a[0] - a[2]) * (b[0] + b[3]);
  float zz = (a[0] + a[2]) * (b[0] - b[3]);
  float xx = (ww + yy) + zz;
  float qq = 0.5f * (xx + (a[3] - a[1]) * (b[1] - b[2]));
  o[0] = (qq - ww) + (a[3] - a[2]) * (b[2] - b[3]);
  o[1] = (qq - xx) + (a[1] + a[0]) * (b[1] + b[0]);
  o[2] = (qq - yy) + (a[0] - a[1]) * (b[2] + b[3]);
  o[3] = (qq - zz) + (a[3] + a[2]) * (b[0] - b[1]);
}

// the command of the squashed action u (action_scale, diff_action.py:174-176)
GR_HD void gr_diff_command(const gr_diff_consts& k, const gr_diff_env& e, float sc[4], float cmd[4]) {
  float weight = e.mc * k.gravity;
  float s0 = (weight * k.thrust_ratio) / 2.0f;
  float of[4];
  sc[0] = s0; of[0] = s0;
  for (int i = 1; i < 4; ++i) { sc[i] = k.rate_bound; of[i] = 0.0f; }
  for (int i = 0; i < 4; ++i) cmd[i] = e.u[i] * sc[i] + of[i];
  cmd[0] = cmd[0] * e.thr;
}

// The step's forward: tt = (T+, tau+), then x+ in place of e.p / e.q / e.v / e.w (ctbr_compute<NO_MOTOR>, dd_explicit).
GR_HD void gr_diff_forward(const gr_diff_consts& k, gr_diff_env& e, float tt[4]) {
  float sc[4], cmd[4];
  gr_diff_command(k, e, sc, cmd);
  // ---- ctbr_compute<NO_MOTOR>
  float T_des = gr_clampf(cmd[0], k.thrust_lo, k.thrust_hi);
  float T = (1.0f - e.cT) * T_des + e.cT * e.T;
  const float* Jn = k.inertia;
  float err[3], Jw[3], cr[3], tau[3];
  for (int i = 0; i < 3; ++i) err[i] = gr_clampf(cmd[i + 1], -k.rate_bound, k.rate_bound) - e.w[i];
  for (int i = 0; i < 3; ++i) Jw[i] = Jn[i] * e.w[i];
  gr_diff_cross3(e.w, Jw, cr);
  for (int i = 0; i < 3; ++i) {
    float tdes = (Jn[i] * (e.Kp[i] * err[i]) + cr[i]) - e.Kd[i] * e.al[i];
    tau[i] = (1.0f - e.ct[i]) * tdes + e.ct[i] * e.tau[i];
  }
  tt[0] = T; tt[1] = tau[0]; tt[2] = tau[1]; tt[3] = tau[2];
  // ---- dd_explicit
  const float m = k.dr_plant ? e.mp : e.mc;
  float J[3];
  for (int i = 0; i < 3; ++i) J[i] = k.dr_plant ? e.J[i] : k.inertia[i];
  const float dt = k.dt;
  float* p = e.p; float* q = e.q; float* v = e.v; float* w = e.w;
  float vb[3];
  gr_diff_quat_rotate_inverse(q, v, vb);
  float thr[3] = {0.0f, 0.0f, tt[0]};
  for (int i = 0; i < 3; ++i) thr[i] = (thr[i] - (e.k2[i] * vb[i]) * gr_fabsf(vb[i])) - e.k1[i] * vb[i];
  float tw[3];
  gr_diff_quat_rotate(q, thr, tw);
  float acc[3] = {0.0f + tw[0] / m, 0.0f + tw[1] / m, -k.gravity + tw[2] / m};
  float Jpw[3] = {J[0] * w[0], J[1] * w[1], J[2] * w[2]}, crp[3];
  gr_diff_cross3(w, Jpw, crp);
  float al[3];
  for (int i = 0; i < 3; ++i) {
    float ji = 1.0f / J[i];
    al[i] = ji * tt[i + 1] - ji * crp[i];
  }
  for (int i = 0; i < 3; ++i) p[i] = (p[i] + v[i] * dt) + ((0.5f * acc[i]) * dt) * dt;
  float wq[4] = {0.0f, w[0], w[1], w[2]}, qd[4];
  gr_diff_quat_mul(q, wq, qd);
  for (int i = 0; i < 4; ++i) q[i] = q[i] + (0.5f * qd[i]) * dt;
  float nq = gr_sqrtf(((q[0] * q[0] + q[1] * q[1]) + q[2] * q[2]) + q[3] * q[3]);
  for (int i = 0; i < 4; ++i) q[i] = q[i] / nq;
  for (int i = 0; i < 3; ++i) v[i] = v[i] + acc[i] * dt;
  for (int i = 0; i < 3; ++i) w[i] = w[i] + al[i] * dt;
}

// The three weighted loss terms on the post-step state (losses.py:72-117; weights of LossesCfg).
GR_HD void gr_diff_loss_terms(const gr_diff_consts& k, const float pp[3], const float vp[3], const float g[3],
                              float terms[3]) {
  float d[3] = {g[0] - pp[0], g[1] - pp[1], g[2] - pp[2]};
  float dist = gr_sqrtf((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
  float vel = ((vp[0] * vp[0] + vp[1] * vp[1]) + vp[2] * vp[2]) / 3.0f;
  float z = pp[2];
  float fall = 1.0f / ((1.0f + 1.0f * z) + 10.0f * (z * z));
  terms[0] = k.w_target * dist;
  terms[1] = k.w_vel * vel;
  terms[2] = k.w_fall * fall;
}

// The adjoints a window carries backwards for one env: of the pre-step state of the step after, and of its filters.
struct gr_diff_adj {
  float p[3], q[4], v[3], w[3], T, tau[3];
};

// One step of the reverse sweep.  On entry `a` holds the adjoints that come back from step t + 1; on return those of
// step t's pre-step state and filters.  e: the step's pre-step fields; pp / qp / vp: its post-step p+, q+, v+; g: the
// gate centre the loss was taken against; done: the step reset the env (the adjoints from t + 1 are cut; the step's own
// loss still differentiates).  ga: the step's dL/da for the action that produced e.u.
GR_HD void gr_diff_backward(const gr_diff_consts& k, const gr_diff_env& e, const float pp[3], const float qp[4],
                            const float vp[3], const float g[3], bool done, float scale, gr_diff_adj& a, float ga[4]) {
  if (done) {
    for (int i = 0; i < 3; ++i) { a.p[i] = 0.0f; a.v[i] = 0.0f; a.w[i] = 0.0f; a.tau[i] = 0.0f; }
    for (int i = 0; i < 4; ++i) a.q[i] = 0.0f;
    a.T = 0.0f;
  }
  // ---- the loss's gradient at x+ (||.|| has gradient 0 at 0), then the alignment's decay
  float d[3] = {pp[0] - g[0], pp[1] - g[1], pp[2] - g[2]};
  float dist = gr_sqrtf((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
  float idist = dist > 0.0f ? (k.w_target * scale) / dist : 0.0f;
  float z = pp[2];
  float den = (1.0f + z) + 10.0f * (z * z);
  float lp[3], lq[4], lv[3], lw[3];
  for (int i = 0; i < 3; ++i) lp[i] = d[i] * idist;
  lp[2] = lp[2] - ((k.w_fall * scale) * (1.0f + 20.0f * z)) / (den * den);
  for (int i = 0; i < 3; ++i) lv[i] = ((k.w_vel * scale) * (2.0f / 3.0f)) * vp[i];
  for (int i = 0; i < 3; ++i) { lp[i] = k.gamma * (lp[i] + a.p[i]); lv[i] = k.gamma * (lv[i] + a.v[i]); lw[i] = k.gamma * a.w[i]; }
  for (int i = 0; i < 4; ++i) lq[i] = k.gamma * a.q[i];
  // ---- dd_explicit's adjoint at the pre-step state
  const float m = k.dr_plant ? e.mp : e.mc;
  float J[3];
  for (int i = 0; i < 3; ++i) J[i] = k.dr_plant ? e.J[i] : k.inertia[i];
  const float dt = k.dt;
  const float* q = e.q;
  const float* w = e.w;
  float ap[3], aq[4], av[3], aw[3], lacc[3], lal[3];
  for (int i = 0; i < 3; ++i) {
    ap[i] = lp[i];
    av[i] = lp[i] * dt + lv[i];
    lacc[i] = (0.5f * dt * dt) * lp[i] + dt * lv[i];
    aw[i] = lw[i];
    lal[i] = dt * lw[i];
  }
  // q+ = qn / |qn|, qn = q + 0.5 dt q (x) (0, w)
  float wq[4] = {0.0f, w[0], w[1], w[2]}, qd[4], qn[4];
  gr_diff_quat_mul(q, wq, qd);
  for (int i = 0; i < 4; ++i) qn[i] = q[i] + (0.5f * qd[i]) * dt;
  float nq = gr_sqrtf(((qn[0] * qn[0] + qn[1] * qn[1]) + qn[2] * qn[2]) + qn[3] * qn[3]);
  float qdot = ((qp[0] * lq[0] + qp[1] * lq[1]) + qp[2] * lq[2]) + qp[3] * lq[3];
  float lqn[4];
  for (int i = 0; i < 4; ++i) lqn[i] = (lq[i] - qp[i] * qdot) / nq;
  // c = a (x) b: adjoint of a is lc (x) conj(b), of b is conj(a) (x) lc
  float wqc[4] = {0.0f, -w[0], -w[1], -w[2]}, qc[4] = {q[0], -q[1], -q[2], -q[3]}, t4[4], u4[4];
  gr_diff_quat_mul(lqn, wqc, t4);
  gr_diff_quat_mul(qc, lqn, u4);
  for (int i = 0; i < 4; ++i) aq[i] = lqn[i] + (0.5f * dt) * t4[i];
  for (int i = 0; i < 3; ++i) aw[i] = aw[i] + (0.5f * dt) * u4[i + 1];
  // al = (tau+ - w x Jw) / J
  float ltt[4], lcr[3], Jw[3], t3[3], lb[3];
  for (int i = 0; i < 3; ++i) { ltt[i + 1] = lal[i] / J[i]; lcr[i] = -(lal[i] / J[i]); Jw[i] = J[i] * w[i]; }
  gr_diff_cross3(Jw, lcr, t3);
  gr_diff_cross3(lcr, w, lb);
  for (int i = 0; i < 3; ++i) aw[i] = (aw[i] + t3[i]) + J[i] * lb[i];
  // acc = g + R(q) f / m, f = (0, 0, T+) - k2 vb |vb| - k1 vb, vb = R(q)^T v (as the explicit, un-normalised formulas)
  float vb[3], f[3], ltw[3], lf[3], lvb[3];
  gr_diff_quat_rotate_inverse(q, e.v, vb);
  // T+ of this step is needed for f: recomputed below from the controller (the clamp's pass flags come with it)
  float sc[4], cmd[4];
  gr_diff_command(k, e, sc, cmd);
  const bool pass0 = cmd[0] >= k.thrust_lo && cmd[0] <= k.thrust_hi;
  float Tp = (1.0f - e.cT) * gr_clampf(cmd[0], k.thrust_lo, k.thrust_hi) + e.cT * e.T;
  f[0] = 0.0f; f[1] = 0.0f; f[2] = Tp;
  for (int i = 0; i < 3; ++i) f[i] = (f[i] - (e.k2[i] * vb[i]) * gr_fabsf(vb[i])) - e.k1[i] * vb[i];
  for (int i = 0; i < 3; ++i) ltw[i] = lacc[i] / m;
  gr_diff_quat_rotate_inverse(q, ltw, lf);  // M(q)^T ltw
  const float* qv = q + 1;
  float c3[3];
  gr_diff_cross3(qv, f, c3);
  float lqw = (4.0f * q[0]) * gr_diff_dot3(f, ltw) + 2.0f * gr_diff_dot3(c3, ltw);
  gr_diff_cross3(f, ltw, c3);
  float qf = gr_diff_dot3(qv, f), ql = gr_diff_dot3(qv, ltw);
  float lqv[3];
  for (int i = 0; i < 3; ++i) lqv[i] = (2.0f * q[0]) * c3[i] + 2.0f * (qf * ltw[i] + ql * f[i]);
  ltt[0] = lf[2];
  for (int i = 0; i < 3; ++i) lvb[i] = -(lf[i] * ((2.0f * e.k2[i]) * gr_fabsf(vb[i]) + e.k1[i]));
  float rv[3];
  gr_diff_quat_rotate(q, lvb, rv);  // Minv(q)^T lvb
  for (int i = 0; i < 3; ++i) av[i] = av[i] + rv[i];
  gr_diff_cross3(qv, e.v, c3);
  lqw = (lqw + (4.0f * q[0]) * gr_diff_dot3(e.v, lvb)) - 2.0f * gr_diff_dot3(c3, lvb);
  gr_diff_cross3(e.v, lvb, c3);
  float qvv = gr_diff_dot3(qv, e.v), qlv = gr_diff_dot3(qv, lvb);
  for (int i = 0; i < 3; ++i) lqv[i] = (lqv[i] - (2.0f * q[0]) * c3[i]) + 2.0f * (qvv * lvb[i] + qlv * e.v[i]);
  aq[0] = aq[0] + lqw;
  for (int i = 0; i < 3; ++i) aq[i + 1] = aq[i + 1] + lqv[i];
  // ---- the filters (their adjoints are carried undecayed) and the controller; w_b and alpha_b enter detached
  const float lT = a.T + ltt[0];
  float ltau[3], lcmd[4];
  for (int i = 0; i < 3; ++i) ltau[i] = a.tau[i] + ltt[i + 1];
  lcmd[0] = pass0 ? (1.0f - e.cT) * lT : 0.0f;
  for (int i = 0; i < 3; ++i) {
    const bool pass = cmd[i + 1] >= -k.rate_bound && cmd[i + 1] <= k.rate_bound;
    lcmd[i + 1] = pass ? ((1.0f - e.ct[i]) * (k.inertia[i] * e.Kp[i])) * ltau[i] : 0.0f;
  }
  lcmd[0] = lcmd[0] * e.thr;
  for (int i = 0; i < 4; ++i) ga[i] = (lcmd[i] * sc[i]) * (1.0f - e.u[i] * e.u[i]);
  a.T = e.cT * lT;
  for (int i = 0; i < 3; ++i) a.tau[i] = e.ct[i] * ltau[i];
  for (int i = 0; i < 3; ++i) { a.p[i] = ap[i]; a.v[i] = av[i]; a.w[i] = aw[i]; }
  for (int i = 0; i < 4; ++i) a.q[i] = aq[i];
}
