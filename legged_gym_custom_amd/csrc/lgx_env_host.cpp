// lgx_env_host.cpp — host (CPU) backend of the env step behind include/lgx.h
// (lgx_create(device = -1); the reference's `--sim_device=cpu`, helpers.py:174-177, config
// C1). Same entry points, buffers and semantics as the HIP kernels of lgx_env.hip; the
// algorithm is the kernel's (DESIGN.md §3 physics spec), laid out for a CPU core:
//   * one OpenMP thread steps one env at a time (dynamic schedule: contact counts vary);
//   * the env's working set (`Env`, ~25 KB with the dense constraint matrix) stays in the
//     thread's L1/L2 for the whole step, as the kernel keeps it in LDS;
//   * the kernel's lane-parallel phases become short loops in the kernel's order: links
//     base-to-tip, joints 0..11, constraint rows [joint limits | 3 per contact];
//   * the constraint solve always uses the dense A = J M⁻¹ Jᵀ (the kernel switches to a
//     velocity-space sweep above 24 rows to bound LDS; both are the same Gauss-Seidel).
// Post-physics follows legged_robot.py / go2.py statement order with no fp contraction
// (built with -ffp-contract=off), like the kernel's golden-pinned tail. The scalar code with
// no lane index in it is the kernel's own, from lgx_env_common.h; what stays here is the physics
// and the phases the kernel runs lane-parallel.
#include <math.h>
#include <cmath>
#include <omp.h>
#include <stdint.h>
#include <string.h>

#include <algorithm>
#include <initializer_list>
#include <vector>

#include "lgx_env_common.h"
#include "lgx_host.h"

namespace lgxh {

using namespace lgx;  // the shared scalar code (lgx_env_common.h)

// ------------------------------------------------------------------ per-env state
struct Link {
  float R[9], P[3], ax[3], W[3], V[3], C[3], I[6], m, F[3], N[3];
};
struct Env {
  // physics (base velocity held as the ORIGIN velocity inside the step)
  float qb[4], pb[3], vo[3], wb[3];
  float th[NJ], thd[NJ], tau[NJ], act[NJ], kpm[NJ], kdm[NJ], ldv[NJ];
  float madd, cadd[3], mu;
  int fon;                                     // external force (ABI 16): on in this step,
  float fw[3], fpt[3];                         // world vector, application point (base link frame)
  Link lk[NL];
  float tot[16];                               // base sums about p0: m, h(3), Ip(6), F(3), N(3)
  float hj[NJ], Bc[NJ][6], Dl[4][6], Dinv[4][6], X[NJ][6], Sinv[6][6], hb[6];
  float us[NU], up[NU];
  int nrows, nlim, ncon;
  float J[MAXR][9], ZG[MAXR][9];               // sparse rows [base 6 | leg 3]; z_r (6) | g_r (3)
  float Arr[MAXR], tgt[MAXR], lam[MAXR], w[MAXR];
  int rleg[MAXR];
  int cbody[MAXC];
  float cn[MAXC][3];
  float A[MAXR * MAXR];
  float cf[LGX_MAX_BODIES][3], rbz[LGX_MAX_BODIES];
  // post-physics
  float root[13], cmd[4], U[4 * NBLK_MAX];
  Scratch x;
  int lc[4];
  float lch[4], fat[4];
  float cur[LGX_MAX_PROPRIO], hist[MAXHIST], heights[LGX_MAX_HEIGHT_POINTS];
  float jsum[16], rterm[64];
  long long ep;
  int reset, tout;
};

// ------------------------------------------------------------------ kinematics
// Links base to tip (chain position 0..2 of each leg after the base): world rotation,
// origin, joint axis, angular velocity, COM; with BIAS the velocity-product accelerations
// and per-link COM wrench plus the 16 base sums about p0; without, the origin velocities.
template <bool BIAS>
static void kinematics(Env& s, const lgx_model* M, const lgx_task_params* P) {
  float Al[NL][3], Ao[NL][3];
  {
    Link& b = s.lk[0];
    quat_to_R(s.qb, b.R);
    st3(b.P, ld3(s.pb)); st3(b.ax, mk(0, 0, 0)); st3(b.W, ld3(s.wb)); st3(b.V, ld3(s.vo));
    st3(Al[0], mk(0, 0, 0)); st3(Ao[0], mk(0, 0, 0));
  }
  for (int j = 0; j < NJ; ++j) {
    const int k = j + 1, par = (j % 3 == 0) ? 0 : j;
    const Link& p = s.lk[par];
    Link& c = s.lk[k];
    const f3 orig = ld3(M->joint_origin[k]), al = ld3(M->joint_axis[k]);
    const float* Rj = M->joint_rot[k];
    const float th = s.th[j], ct = cosf(th), st = sinf(th), t1 = 1.f - ct;
    const float Ra[9] = {t1 * al.x * al.x + ct, t1 * al.x * al.y - st * al.z, t1 * al.x * al.z + st * al.y,
                         t1 * al.x * al.y + st * al.z, t1 * al.y * al.y + ct, t1 * al.y * al.z - st * al.x,
                         t1 * al.x * al.z - st * al.y, t1 * al.y * al.z + st * al.x, t1 * al.z * al.z + ct};
    float Rl[9];
    mm(Rj, Ra, Rl);
    const f3 o = mv(p.R, orig), ax = mv(p.R, mv(Rj, al));
    mm(p.R, Rl, c.R);
    const f3 Wp = ld3(p.W), wa = ax * s.thd[j];
    st3(c.P, ld3(p.P) + o);
    st3(c.ax, ax);
    st3(c.W, Wp + wa);
    if constexpr (BIAS) {
      st3(Al[k], ld3(Al[par]) + cross(Wp, wa));
      st3(Ao[k], ld3(Ao[par]) + cross(ld3(Al[par]), o) + cross(Wp, cross(Wp, o)));
    } else {
      st3(c.V, ld3(p.V) + cross(Wp, o));
    }
  }
  const f3 g = ld3(P->gravity), p0 = ld3(s.pb);
  if constexpr (BIAS) memset(s.tot, 0, sizeof(s.tot));
  for (int k = 0; k < NL; ++k) {
    Link& c = s.lk[k];
    const float cb = k == 0 ? 1.f : 0.f;
    const float* cl = M->link_com[k];
    const f3 C = ld3(c.P) + mv(c.R, mk(cl[0] + cb * s.cadd[0], cl[1] + cb * s.cadd[1], cl[2] + cb * s.cadd[2]));
    st3(c.C, C);
    if constexpr (BIAS) {
      const float m = M->link_mass[k] + cb * s.madd;
      const float* In = M->link_inertia[k];
      const float Il[9] = {In[0], In[3], In[4], In[3], In[1], In[5], In[4], In[5], In[2]};
      const float* R = c.R;
      float T[9];
      mm(R, Il, T);
      float* Iw = c.I;
      Iw[0] = T[0] * R[0] + T[1] * R[1] + T[2] * R[2];
      Iw[1] = T[3] * R[3] + T[4] * R[4] + T[5] * R[5];
      Iw[2] = T[6] * R[6] + T[7] * R[7] + T[8] * R[8];
      Iw[3] = T[0] * R[3] + T[1] * R[4] + T[2] * R[5];
      Iw[4] = T[0] * R[6] + T[1] * R[7] + T[2] * R[8];
      Iw[5] = T[3] * R[6] + T[4] * R[7] + T[5] * R[8];
      c.m = m;
      const f3 W = ld3(c.W), al = ld3(Al[k]), rl = C - ld3(c.P);
      const f3 acc = ld3(Ao[k]) + cross(al, rl) + cross(W, cross(W, rl));
      f3 F = (acc - g) * m, N = symv(Iw, al) + cross(W, symv(Iw, W));
      // external force (include/lgx.h, ABI 16): on the base link, at a = P0 + R0 * point
      if (k == 0 && s.fon) {
        const f3 f = ld3(s.fw);
        F = F - f;
        N = N - cross(ld3(c.P) + mv(R, ld3(s.fpt)) - C, f);
      }
      st3(c.F, F);
      st3(c.N, N);
      const f3 r = C - p0;
      const float rr = dot(r, r);
      const f3 Nt = cross(r, F) + N;
      const float rd[16] = {m, m * r.x, m * r.y, m * r.z,
                            Iw[0] + m * (rr - r.x * r.x), Iw[1] + m * (rr - r.y * r.y), Iw[2] + m * (rr - r.z * r.z),
                            Iw[3] - m * r.x * r.y, Iw[4] - m * r.x * r.z, Iw[5] - m * r.y * r.z,
                            F.x, F.y, F.z, Nt.x, Nt.y, Nt.z};
      for (int q = 0; q < 16; ++q) s.tot[q] += rd[q];
    }
  }
}

// Mass matrix M = [A B; Bᵀ D] (D block diagonal over the legs) and bias h, factored:
// X = B D⁻¹, S = A − X Bᵀ (base Schur complement), S⁻¹ — lgx_env.hip `dynamics`.
static void dynamics(Env& s) {
  const f3 p0 = ld3(s.lk[0].P);
  for (int j = 0; j < NJ; ++j) {
    const int l = j / 3, a = j % 3;
    const Link& lj = s.lk[1 + j];
    const f3 ax = ld3(lj.ax), pj = ld3(lj.P);
    f3 acc = mk(0, 0, 0), hl = mk(0, 0, 0), bang = mk(0, 0, 0);
    for (int i = a; i < 3; ++i) {
      const Link& c = s.lk[1 + 3 * l + i];
      const f3 C = ld3(c.C), d = C - pj;
      acc = acc + cross(d, ld3(c.F)) + ld3(c.N);
      hl = hl + d * c.m;
      bang = bang + cross(C - p0, cross(ax, d)) * c.m + symv(c.I, ax);
    }
    s.hj[j] = dot(ax, acc);
    const f3 blin = cross(ax, hl);
    float* Bj = s.Bc[j];
    Bj[0] = blin.x; Bj[1] = blin.y; Bj[2] = blin.z; Bj[3] = bang.x; Bj[4] = bang.y; Bj[5] = bang.z;
  }
  for (int l = 0; l < 4; ++l) {
    for (int e = 0; e < 6; ++e) {
      const int j1 = e < 3 ? e : (e == 5 ? 1 : 0), j2 = e < 3 ? e : (e == 3 ? 1 : 2);
      const Link& k1 = s.lk[1 + 3 * l + j1];
      const Link& k2 = s.lk[1 + 3 * l + j2];
      const f3 a1 = ld3(k1.ax), a2 = ld3(k2.ax), q1 = ld3(k1.P), q2 = ld3(k2.P);
      float acc = 0.f;
      for (int i = j2; i < 3; ++i) {
        const Link& c = s.lk[1 + 3 * l + i];
        const f3 C = ld3(c.C);
        acc += c.m * dot(cross(a1, C - q1), cross(a2, C - q2)) + dot(a1, symv(c.I, a2));
      }
      s.Dl[l][e] = acc;
    }
    sym3_inv(s.Dl[l], s.Dinv[l]);
  }
  for (int j = 0; j < NJ; ++j) {
    const int l = j / 3, a = j % 3;
    const float d0 = sym3(s.Dinv[l], a, 0), d1 = sym3(s.Dinv[l], a, 1), d2 = sym3(s.Dinv[l], a, 2);
    for (int r = 0; r < 6; ++r) s.X[j][r] = d0 * s.Bc[3 * l][r] + d1 * s.Bc[3 * l + 1][r] + d2 * s.Bc[3 * l + 2][r];
  }
  const float* t = s.tot;
  const float Mt = t[0], Hx = t[1], Hy = t[2], Hz = t[3];
  const float Ab[21] = {Mt, 0.f, Mt, 0.f, 0.f, Mt, 0.f, -Hz, Hy, t[4], Hz, 0.f, -Hx, t[7], t[5],
                        -Hy, Hx, 0.f, t[8], t[9], t[6]};
  float L[21];
  for (int q = 0; q < 21; ++q) {
    const int r = (q >= 1) + (q >= 3) + (q >= 6) + (q >= 10) + (q >= 15), c = q - r * (r + 1) / 2;
    float acc = 0.f;
    for (int j = 0; j < NJ; ++j) acc += s.X[j][r] * s.Bc[j][c];
    L[q] = Ab[q] - acc;
  }
  float inv[6];
  for (int c = 0; c < 6; ++c) {  // Cholesky S = L Lᵀ (packed lower)
    float d = L[pk(c, c)];
    for (int k = 0; k < c; ++k) d -= L[pk(c, k)] * L[pk(c, k)];
    inv[c] = 1.0f / sqrtf(fmaxf(d, 1e-12f));
    for (int r = c + 1; r < 6; ++r) {
      float v = L[pk(r, c)];
      for (int k = 0; k < c; ++k) v -= L[pk(r, k)] * L[pk(c, k)];
      L[pk(r, c)] = v * inv[c];
    }
  }
  for (int col = 0; col < 6; ++col) {  // S⁻¹ e_col
    float x[6];
    for (int r = 0; r < 6; ++r) {
      float v = r == col ? 1.f : 0.f;
      for (int k = 0; k < r; ++k) v -= L[pk(r, k)] * x[k];
      x[r] = v * inv[r];
    }
    for (int r = 5; r >= 0; --r) {
      float v = x[r];
      for (int k = r + 1; k < 6; ++k) v -= L[pk(k, r)] * x[k];
      x[r] = v * inv[r];
    }
    for (int r = 0; r < 6; ++r) s.Sinv[col][r] = x[r];
  }
  for (int q = 0; q < 6; ++q) s.hb[q] = t[10 + q];
}

// ------------------------------------------------------------------ terrain contact
// The reference's trimesh (terrain_utils.py:382-465) rebuilt per query from the packed
// per-vertex words (height | wall shift), as lgx_env.hip terrain_contact.
// penetration depth (> 0 overlapping) and unit normal (terrain -> sphere) at x, radius r
static float terrain_contact(const lgx_task_params* P, const lgx_buffers* B, f3 x, float r, f3& n) {
  const float hs = P->horizontal_scale, vs = P->vertical_scale;
  const int rows = P->hf_rows, cols = P->hf_cols;
  const float gx = x.x + P->border_size, gy = x.y + P->border_size;
  const int ci = (int)floorf(gx / hs), cj = (int)floorf(gy / hs);
  const f3 p = mk(gx - (float)ci * hs, gy - (float)cj * hs, x.z);
  const int i0 = std::max(ci + (int)ceilf((p.x - r) / hs) - 2, 0), i1 = std::min(ci + (int)floorf((p.x + r) / hs) + 1, rows - 2);
  const int j0 = std::max(cj + (int)ceilf((p.y - r) / hs) - 2, 0), j1 = std::min(cj + (int)floorf((p.y + r) / hs) + 1, cols - 2);
  float best = 3.0e38f, zs = -3.0e38f;
  f3 q = mk(0.f, 0.f, -3.0e38f), fn = mk(0.f, 0.f, 1.f);
  for (int i = i0; i <= i1; ++i)
    for (int j = j0; j <= j1; ++j) {
      const f3 v00 = mesh_vertex(B->terrain_mesh, cols, i, j, ci, cj, hs, vs);
      const f3 v01 = mesh_vertex(B->terrain_mesh, cols, i, j + 1, ci, cj, hs, vs);
      const f3 v10 = mesh_vertex(B->terrain_mesh, cols, i + 1, j, ci, cj, hs, vs);
      const f3 v11 = mesh_vertex(B->terrain_mesh, cols, i + 1, j + 1, ci, cj, hs, vs);
      for (int t = 0; t < 2; ++t) {
        const f3 a = v00, b = t == 0 ? v11 : v10, c = t == 0 ? v01 : v11;
        const f3 cp = closest_on_triangle(p, a, b, c), d = p - cp;
        const float d2 = dot(d, d);
        if (d2 < best) { best = d2; q = cp; fn = cross(b - a, c - a); }
        float z;
        if (height_in_triangle(p, a, b, c, z)) zs = fmaxf(zs, z);
      }
    }
  if (best >= 3.0e38f) {
    n = mk(0.f, 0.f, 1.f);
    return -3.0e38f;
  }
  const float dist = sqrtf(best);
  const bool below = p.z < zs;
  n = dist > 1e-6f ? (p - q) * ((below ? -1.0f : 1.0f) / dist) : fn * (1.0f / sqrtf(fmaxf(dot(fn, fn), 1e-30f)));
  return below ? r + dist : r - dist;
}
// not shared with the kernel's contact_tangents: this one divides by sqrtf(l2), the kernel uses rsqrtf(l2)
static void tangents(f3 n, f3& t1, f3& t2) {
  f3 a = mk(n.z, 0.f, -n.x);
  float l2 = a.x * a.x + a.z * a.z;
  if (l2 < 1e-8f) {
    a = mk(0.f, n.z, -n.y);
    l2 = a.y * a.y + a.z * a.z;
  }
  t1 = a * (1.0f / sqrtf(l2));
  t2 = cross(n, t1);
}

// ------------------------------------------------------------------ SEA actuator net
// anymal.py:71-81: 2-layer LSTM(2 -> 8 -> 8) (gates i f g o), Linear(8 -> 1); state
// [2, N*D, 8] in the caller's buffers.
static inline float sigm(float x) { return 1.0f / (1.0f + expf(-x)); }
static void lstm_cell(const float* w_ih, int nin, const float* w_hh, const float* b_ih, const float* b_hh,
                      const float* x, float* h, float* c) {
  float hn[8];
  for (int u = 0; u < 8; ++u) {
    float g4[4];
    for (int q = 0; q < 4; ++q) {
      const int g = q * 8 + u;
      float a = 0.0f, b = 0.0f;
      for (int k = 0; k < nin; ++k) a += w_ih[g * nin + k] * x[k];
      for (int k = 0; k < 8; ++k) b += w_hh[g * 8 + k] * h[k];
      g4[q] = (a + b_ih[g]) + (b + b_hh[g]);
    }
    c[u] = sigm(g4[1]) * c[u] + sigm(g4[0]) * tanhf(g4[2]);
    hn[u] = sigm(g4[3]) * tanhf(c[u]);
  }
  memcpy(h, hn, sizeof(hn));
}
static float sea_torque(const lgx_task_params* P, const lgx_buffers* B, int e, int j, float in0, float in1) {
  const size_t NT = (size_t)P->num_envs * P->num_dof, r = (size_t)e * P->num_dof + j;
  float* h0 = B->sea_hidden + r * 8;
  float* c0 = B->sea_cell + r * 8;
  float* h1 = B->sea_hidden + (NT + r) * 8;
  float* c1 = B->sea_cell + (NT + r) * 8;
  const float x[2] = {in0 * P->sea_in_scale[0], in1 * P->sea_in_scale[1]};
  lstm_cell(P->sea_w_ih0, 2, P->sea_w_hh0, P->sea_b_ih0, P->sea_b_hh0, x, h0, c0);
  lstm_cell(P->sea_w_ih1, 8, P->sea_w_hh1, P->sea_b_ih1, P->sea_b_hh1, h0, h1, c1);
  float y = 0.0f;
  for (int k = 0; k < 8; ++k) y += P->sea_lin_w[k] * h1[k];
  return P->sea_out_scale * (y + P->sea_lin_b);
}

// ------------------------------------------------------------------ one physics substep
static void substep(Env& s, const lgx_model* M, const lgx_task_params* P, const lgx_buffers* B, int e, int sub,
                    bool last) {
  const float dt = P->sim_dt;
  const bool terrain = P->mesh_type != LGX_MESH_PLANE;
  // PD torques: LeggedRobot._compute_torques legged_robot.py:440-478 (or the SEA net)
  // actuation latency and motor strength (include/lgx.h, ABI 8): the kernel's rule
  int age = 0;
  if (B->action_delay)
    age = action_age(action_delay_clamp(B->action_delay[e], P->action_history_len, P->decimation), sub, P->decimation);
  for (int j = 0; j < NJ; ++j) {
    const float a = (age > 0 && j < P->num_actions)
                        ? B->action_history[((size_t)e * P->action_history_len + (age - 1)) * P->num_actions + j]
                        : s.act[j];
    const float as = a * P->action_scale;
    const float ms = B->motor_strength ? B->motor_strength[(size_t)e * P->num_dof + j] : 1.0f;
    if (P->actuator_net) {
      const float t = sea_torque(P, B, e, j, (as + P->default_dof_pos[j]) - s.th[j], s.thd[j]);
      s.tau[j] = B->motor_strength ? ms * t : t;
      continue;
    }
    float t;
    if (P->control_type == LGX_CONTROL_P) {
      const float err = (as + P->default_dof_pos[j]) - s.th[j];
      t = P->randomize_kp_kd ? (s.kpm[j] * P->p_gains[j]) * err - (s.kdm[j] * P->d_gains[j]) * s.thd[j]
                             : P->p_gains[j] * err - P->d_gains[j] * s.thd[j];
    } else if (P->control_type == LGX_CONTROL_V) {
      t = P->p_gains[j] * (as - s.thd[j]) - P->d_gains[j] * ((s.thd[j] - s.ldv[j]) / P->sim_dt);
    } else {
      t = as;
    }
    if (B->motor_strength) t = ms * t;
    s.tau[j] = fminf(fmaxf(t, -P->torque_limits[j]), P->torque_limits[j]);
  }
  kinematics<true>(s, M, P);
  dynamics(s);
  // free velocity u* = u + dt M⁻¹ [−h_B ; τ − h_J]
  float fj[NJ], vb[6], zb[6];
  for (int j = 0; j < NJ; ++j) fj[j] = s.tau[j] - s.hj[j];
  for (int r = 0; r < 6; ++r) {
    float acc = 0.f;
    for (int j = 0; j < NJ; ++j) acc += s.X[j][r] * fj[j];
    vb[r] = -s.hb[r] - acc;
  }
  for (int r = 0; r < 6; ++r) {
    const float* Si = s.Sinv[r];
    zb[r] = Si[0] * vb[0] + Si[1] * vb[1] + Si[2] * vb[2] + Si[3] * vb[3] + Si[4] * vb[4] + Si[5] * vb[5];
  }
  for (int r = 0; r < 3; ++r) { s.us[r] = s.vo[r] + dt * zb[r]; s.us[3 + r] = s.wb[r] + dt * zb[3 + r]; }
  for (int j = 0; j < NJ; ++j) {
    const int l = j / 3, a = j % 3;
    const float* Di = s.Dinv[l];
    float bot = sym3(Di, a, 0) * fj[3 * l] + sym3(Di, a, 1) * fj[3 * l + 1] + sym3(Di, a, 2) * fj[3 * l + 2];
    for (int r = 0; r < 6; ++r) bot -= s.X[j][r] * zb[r];
    s.us[6 + j] = s.thd[j] + dt * bot;
  }
  // constraint rows: joint limits (joint order), then contacts (candidate order, <= MAXC)
  auto target = [&](float d) {
    if (d > P->slop) return fminf(P->baumgarte * (d - P->slop) / dt, P->max_depenetration_vel);
    return d >= 0.f ? 0.f : d / dt;
  };
  int n = 0;
  for (int j = 0; j < NJ; ++j) {
    if (!M->joint_has_limits[j + 1]) continue;
    const float lo = M->joint_lower[j + 1], hi = M->joint_upper[j + 1];
    const bool llo = s.th[j] < lo + P->limit_margin, lhi = !llo && s.th[j] > hi - P->limit_margin;
    if (!llo && !lhi) continue;
    float* jr = s.J[n];
    memset(jr, 0, sizeof(float) * 9);
    jr[6 + j % 3] = llo ? 1.f : -1.f;
    s.tgt[n] = target(llo ? lo - s.th[j] : s.th[j] - hi);
    s.rleg[n] = j / 3;
    ++n;
  }
  s.nlim = n;
  int nc = 0;
  const f3 p0 = ld3(s.lk[0].P);
  for (int c = 0; c < M->num_candidates && nc < MAXC; ++c) {
    const int ck = M->cand_link[c];
    const Link& lc = s.lk[ck];
    f3 xc = ld3(lc.P) + mv(lc.R, ld3(M->cand_pos[c]));
    const float r = M->cand_radius[c];
    float depth;
    f3 dn = mk(0, 0, 1), d1 = mk(1, 0, 0), d2 = mk(0, 1, 0);
    if (!terrain) {
      depth = r - xc.z;
      xc.z -= r;
    } else {
      depth = terrain_contact(P, B, xc, r, dn);
      xc = xc - dn * r;
      tangents(dn, d1, d2);
    }
    if (!(depth > -P->contact_margin)) continue;
    st3(s.cn[nc], dn);
    const int leg = ck > 0 ? (ck - 1) / 3 : -1, pos = ck > 0 ? (ck - 1) % 3 : -1;
    const int kl = ck > 0 ? 1 + 3 * leg : 1;
    const f3 a0 = ld3(s.lk[kl].ax), a1 = ld3(s.lk[kl + 1].ax), a2 = ld3(s.lk[kl + 2].ax);
    const f3 r0 = xc - ld3(s.lk[kl].P), r1 = xc - ld3(s.lk[kl + 1].P), r2 = xc - ld3(s.lk[kl + 2].P), rb = xc - p0;
    for (int t = 0; t < 3; ++t) {
      const f3 d = t == 0 ? dn : (t == 1 ? d1 : d2), ang = cross(rb, d);
      float* jr = s.J[n];
      jr[0] = d.x; jr[1] = d.y; jr[2] = d.z; jr[3] = ang.x; jr[4] = ang.y; jr[5] = ang.z;
      jr[6] = pos >= 0 ? dot(a0, cross(r0, d)) : 0.f;
      jr[7] = pos >= 1 ? dot(a1, cross(r1, d)) : 0.f;
      jr[8] = pos >= 2 ? dot(a2, cross(r2, d)) : 0.f;
      s.rleg[n] = leg;
      s.tgt[n] = t == 0 ? target(depth) : 0.f;
      ++n;
    }
    s.cbody[nc++] = M->cand_body[c];
  }
  s.ncon = nc;
  s.nrows = n;
  // per row: y = J_B − X_l J_l, z = S⁻¹ y, g = D_l⁻¹ J_l, A_rr, w_r = J_r u*
  float Y[MAXR][6];
  for (int r = 0; r < n; ++r) {
    const float* jr = s.J[r];
    const int lr = s.rleg[r];
    float* y = Y[r];
    float w = 0.f;
    for (int q = 0; q < 6; ++q) { y[q] = jr[q]; w += jr[q] * s.us[q]; }
    float g[3] = {0.f, 0.f, 0.f}, arr = 0.f;
    if (lr >= 0) {
      for (int c = 0; c < 3; ++c) {
        const float* Xc = s.X[3 * lr + c];
        for (int q = 0; q < 6; ++q) y[q] -= Xc[q] * jr[6 + c];
        w += jr[6 + c] * s.us[6 + 3 * lr + c];
      }
      const float* Di = s.Dinv[lr];
      g[0] = Di[0] * jr[6] + Di[3] * jr[7] + Di[4] * jr[8];
      g[1] = Di[3] * jr[6] + Di[1] * jr[7] + Di[5] * jr[8];
      g[2] = Di[4] * jr[6] + Di[5] * jr[7] + Di[2] * jr[8];
      arr = jr[6] * g[0] + jr[7] * g[1] + jr[8] * g[2];
    }
    float* zg = s.ZG[r];
    for (int q = 0; q < 6; ++q) {
      const float* Si = s.Sinv[q];
      zg[q] = Si[0] * y[0] + Si[1] * y[1] + Si[2] * y[2] + Si[3] * y[3] + Si[4] * y[4] + Si[5] * y[5];
      arr += y[q] * zg[q];
    }
    zg[6] = g[0]; zg[7] = g[1]; zg[8] = g[2];
    s.Arr[r] = arr;
    s.lam[r] = 0.f;
    s.w[r] = w;
  }
  // A = J M⁻¹ Jᵀ: A[q][r] = y_r·z_q + [leg_r = leg_q] J_l,r·g_q
  for (int q = 0; q < n; ++q) {
    const float* zg = s.ZG[q];
    for (int r = 0; r < n; ++r) {
      const float* y = Y[r];
      const float* jr = s.J[r];
      const float v = y[0] * zg[0] + y[1] * zg[1] + y[2] * zg[2] + y[3] * zg[3] + y[4] * zg[4] + y[5] * zg[5];
      const float vl = jr[6] * zg[6] + jr[7] * zg[7] + jr[8] * zg[8];
      s.A[q * n + r] = v + (s.rleg[q] == s.rleg[r] ? vl : 0.f);
    }
  }
  // projected Gauss-Seidel: [limits | (normal, tangent pair on the friction disk) per contact]
  float* w = s.w;
  float* lam = s.lam;
  auto apply = [&](int r, float d) {
    const float* Ar = s.A + r * n;
    for (int q = 0; q < n; ++q) w[q] += Ar[q] * d;
  };
  for (int it = 0; it < P->solver_iterations; ++it) {
    for (int r = 0; r < s.nlim; ++r) {
      const float cand = fmaxf(0.f, lam[r] + (s.tgt[r] - w[r]) / s.Arr[r]);
      const float d = cand - lam[r];
      lam[r] = cand;
      apply(r, d);
    }
    for (int r = s.nlim; r < n; r += 3) {
      const float cand = fmaxf(0.f, lam[r] + (s.tgt[r] - w[r]) / s.Arr[r]);
      const float d = cand - lam[r];
      lam[r] = cand;
      apply(r, d);
      const float lim = s.mu * lam[r];
      float l1 = lam[r + 1] - w[r + 1] / s.Arr[r + 1], l2 = lam[r + 2] - w[r + 2] / s.Arr[r + 2];
      const float nn = l1 * l1 + l2 * l2;
      if (nn > lim * lim) {
        const float sc = lim / sqrtf(nn);
        l1 *= sc;
        l2 *= sc;
      }
      const float e1 = l1 - lam[r + 1], e2 = l2 - lam[r + 2];
      lam[r + 1] = l1;
      lam[r + 2] = l2;
      const float* A1 = s.A + (r + 1) * n;
      const float* A2 = s.A + (r + 2) * n;
      for (int q = 0; q < n; ++q) w[q] += A1[q] * e1 + A2[q] * e2;
    }
  }
  // u+ = u* + M⁻¹ Jᵀ λ = u* + [Z ; G_J − Xᵀ Z]
  float Z[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, G[NJ] = {0.f};
  for (int r = 0; r < n; ++r) {
    const float* zg = s.ZG[r];
    for (int q = 0; q < 6; ++q) Z[q] += lam[r] * zg[q];
    if (s.rleg[r] >= 0)
      for (int c = 0; c < 3; ++c) G[3 * s.rleg[r] + c] += lam[r] * zg[6 + c];
  }
  for (int q = 0; q < 6; ++q) s.up[q] = s.us[q] + Z[q];
  for (int j = 0; j < NJ; ++j) {
    float v = s.us[6 + j] + G[j];
    for (int q = 0; q < 6; ++q) v -= s.X[j][q] * Z[q];
    s.up[6 + j] = v;
  }
  // contact forces of the last substep per reported body (world frame)
  if (last) {
    memset(s.cf, 0, sizeof(s.cf));
    for (int c = 0; c < nc; ++c) {
      const int r = s.nlim + 3 * c;
      float* f = s.cf[s.cbody[c]];
      if (!terrain) {
        f[2] += lam[r]; f[0] += lam[r + 1]; f[1] += lam[r + 2];
      } else {
        f3 t1, t2;
        const f3 nrm = ld3(s.cn[c]);
        tangents(nrm, t1, t2);
        const f3 fc = nrm * lam[r] + t1 * lam[r + 1] + t2 * lam[r + 2];
        f[0] += fc.x; f[1] += fc.y; f[2] += fc.z;
      }
    }
    for (int b = 0; b < LGX_MAX_BODIES; ++b)
      for (int i = 0; i < 3; ++i) s.cf[b][i] = s.cf[b][i] / dt;
  }
  // semi-implicit Euler
  const f3 wv = mk(s.up[3], s.up[4], s.up[5]);
  for (int i = 0; i < 3; ++i) s.pb[i] += dt * s.up[i];
  const float wn = sqrtf(dot(wv, wv)), ang = wn * dt;
  float dq[4];
  if (ang > 1e-12f) {
    const float sc = sinf(0.5f * ang) / wn;
    dq[0] = wv.x * sc; dq[1] = wv.y * sc; dq[2] = wv.z * sc; dq[3] = cosf(0.5f * ang);
  } else {
    dq[0] = 0.5f * dt * wv.x; dq[1] = 0.5f * dt * wv.y; dq[2] = 0.5f * dt * wv.z; dq[3] = 1.f;
  }
  const float* q = s.qb;
  float qn[4];
  qn[3] = dq[3] * q[3] - (dq[0] * q[0] + dq[1] * q[1] + dq[2] * q[2]);
  qn[0] = dq[3] * q[0] + q[3] * dq[0] + (dq[1] * q[2] - dq[2] * q[1]);
  qn[1] = dq[3] * q[1] + q[3] * dq[1] + (dq[2] * q[0] - dq[0] * q[2]);
  qn[2] = dq[3] * q[2] + q[3] * dq[2] + (dq[0] * q[1] - dq[1] * q[0]);
  const float nq = 1.0f / sqrtf(qn[0] * qn[0] + qn[1] * qn[1] + qn[2] * qn[2] + qn[3] * qn[3]);
  for (int i = 0; i < 4; ++i) s.qb[i] = qn[i] * nq;
  for (int i = 0; i < 3; ++i) { s.vo[i] = s.up[i]; s.wb[i] = s.up[3 + i]; }
  for (int j = 0; j < NJ; ++j) {
    s.thd[j] = s.up[6 + j];
    s.th[j] += dt * s.thd[j];
  }
}

// ------------------------------------------------------------------ post-physics
// (the helpers, command resampling and reward terms are lgx_env_common.h's)
static void fill_uniforms(Env& s, const lgx_task_params* P, uint64_t seed, uint32_t gid, uint64_t step,
                          uint32_t stream) {
  for (int b = 0; b < rng_blocks(P); ++b) {
    uint32_t o[4];
    philox4x32_10(gid, (uint32_t)step, (uint32_t)b | (stream << 16), (uint32_t)(step >> 32), (uint32_t)seed,
                  (uint32_t)(seed >> 32), o);
    for (int i = 0; i < 4; ++i) s.U[4 * b + i] = u01(o[i]);
  }
}

// reset_idx for env e (go2.py:207-263 / legged_robot.py:157-213) on the env's staged root,
// dof and command state. `stats` (K + 1 floats) receives the episode sums and the count.
static void reset_env(const lgx_task_params* P, const lgx_buffers* B, Env& s, int e, bool zero_carried, float* stats) {
  const int D = P->num_dof;
  const float* U = s.U;
  // an env that resets is built: the terrain curriculum always applies here
  reset_env_head(P, *B, s, U, e, true);
  for (int j = 0; j < D; ++j) {  // legged_robot.py:481-506
    s.th[j] = P->default_dof_pos[j] + rand_range(0.0f, 0.9f, U[S_DOF + j]);
    s.thd[j] = 0.0f;
  }
  if (zero_carried) {
    const int A = P->num_actions, H = P->history_len * P->num_proprio;
    memset(B->last_actions + (size_t)e * A, 0, sizeof(float) * A);
    if (B->action_history)
      memset(B->action_history + (size_t)e * P->action_history_len * A, 0, sizeof(float) * P->action_history_len * A);
    if (B->sensor_count) B->sensor_count[e] = 0;  // sensor model (ABI 15)
    memset(B->last_dof_vel + (size_t)e * D, 0, sizeof(float) * D);
    memset(B->last_torques + (size_t)e * D, 0, sizeof(float) * D);
    memset(B->last_root_vel + (size_t)e * 6, 0, sizeof(float) * 6);
    memset(B->last_base_lin_vel + (size_t)e * 3, 0, sizeof(float) * 3);
    memset(B->obs_history + (size_t)e * H, 0, sizeof(float) * H);
  }
  if (P->actuator_net) {  // anymal.py:56-60
    const size_t NT = (size_t)P->num_envs * D;
    for (int l = 0; l < 2; ++l) {
      memset(B->sea_hidden + (l * NT + (size_t)e * D) * 8, 0, sizeof(float) * 8 * D);
      memset(B->sea_cell + (l * NT + (size_t)e * D) * 8, 0, sizeof(float) * 8 * D);
    }
  }
  if (P->task_kind == LGX_TASK_GO2)
    for (int f = 0; f < P->num_feet; ++f) {
      if (B->feet_air_time) B->feet_air_time[e * P->num_feet + f] = 0.f;
      B->last_contacts[e * P->num_feet + f] = 0;
      B->last_contact_heights[e * P->num_feet + f] = 0.f;
    }
  const int K = P->num_reward_terms + (P->has_termination_reward ? 1 : 0);
  float* es = B->episode_sums + (size_t)e * K;
  // the command curriculum's input (go2.py:87): the tracking_lin_vel sum at an in-step reset
  if (!zero_carried && B->curriculum_vals) B->curriculum_vals[e] = es[P->curriculum_term];
  for (int k = 0; k < K; ++k) {
    stats[k] = es[k];
    es[k] = 0.f;
  }
  stats[K] = 1.0f;
}

// LeggedRobot._get_heights legged_robot.py:997-1032
static void get_heights(const lgx_task_params* P, const lgx_buffers* B, Env& s) {
  const int NP = P->num_height_points;
  if (P->mesh_type == LGX_MESH_PLANE || B->height_samples == nullptr) {
    for (int i = 0; i < NP; ++i) s.heights[i] = 0.0f;
    return;
  }
  const float* root = s.root;
  float qy[4];
  scan_yaw_quat(root[5], root[6], qy);
  for (int i = 0; i < NP; ++i)
    s.heights[i] = scan_point_height(P, B->height_samples, qy, root, P->height_points[i][0],
                                     P->height_points[i][1]);
}

// sums over joints / height points shared by the reward terms (lgx_env.hip joint_sums)
static void joint_sums(const lgx_task_params* P, const lgx_buffers* B, Env& s, int e) {
  const int D = P->num_dof, A = P->num_actions;
  for (int k = 0; k < J_N; ++k) s.jsum[k] = 0.f;
  for (int j = 0; j < D; ++j) {
    const float la = B->last_actions[(size_t)e * A + j], lt = B->last_torques[(size_t)e * D + j];
    const float q = s.th[j], qd = s.thd[j], tau = s.tau[j], dq = q - P->default_dof_pos[j];
    s.jsum[J_ACTION_RATE] += sq(la - s.act[j]);
    s.jsum[J_DELTA_TORQUES] += sq(tau - lt);
    s.jsum[J_DOF_ACC] += sq((s.ldv[j] - qd) / P->dt);
    s.jsum[J_DOF_ERROR] += sq(dq);
    const float lo = q - P->dof_pos_limits[j][0], hi = q - P->dof_pos_limits[j][1];
    float o = -(lo < 0.0f ? lo : 0.0f);
    o += (hi > 0.0f ? hi : 0.0f);
    s.jsum[J_DOF_POS_LIMITS] += o;
    s.jsum[J_DOF_VEL] += sq(qd);
    s.jsum[J_DOF_VEL_LIMITS] += clipf(fabsf(qd) - P->dof_vel_limits[j] * P->soft_dof_vel_limit, 0.0f, 1.0f);
    s.jsum[J_STAND_ABS] += fabsf(dq);
    const float t = fabsf(tau) - P->torque_limits[j] * P->soft_torque_limit;
    s.jsum[J_TORQUE_LIMITS] += t > 0.0f ? t : 0.0f;
    s.jsum[J_TORQUES] += sq(tau);
    for (int i = 0; i < 4; ++i) {
      if (P->hip_joint_idx[i] == j) s.jsum[J_HIP_POS] += sq(dq);
      if (P->thigh_joint_idx[i] == j) s.jsum[J_THIGH_POS] += sq(dq);
      if (P->calf_joint_idx[i] == j) s.jsum[J_CALF_POS] += sq(dq);
    }
  }
  for (int i = 0; i < P->num_height_points; ++i) s.jsum[J_HEIGHT] += s.root[2] - s.heights[i];
}

static inline float fnorm(const float* c) { return nrm3(c[0], c[1], c[2]); }

// rotation matrix -> quaternion xyzw with w >= 0 (rigid-body state tensor)
static void mat_quat(const float* Rb, float* qq) {
  const float tr = Rb[0] + Rb[4] + Rb[8];
  if (tr > 0.f) {
    const float sc = sqrtf(tr + 1.f) * 2.f;
    qq[3] = 0.25f * sc; qq[0] = (Rb[7] - Rb[5]) / sc; qq[1] = (Rb[2] - Rb[6]) / sc; qq[2] = (Rb[3] - Rb[1]) / sc;
  } else if (Rb[0] > Rb[4] && Rb[0] > Rb[8]) {
    const float sc = sqrtf(1.f + Rb[0] - Rb[4] - Rb[8]) * 2.f;
    qq[3] = (Rb[7] - Rb[5]) / sc; qq[0] = 0.25f * sc; qq[1] = (Rb[1] + Rb[3]) / sc; qq[2] = (Rb[2] + Rb[6]) / sc;
  } else if (Rb[4] > Rb[8]) {
    const float sc = sqrtf(1.f + Rb[4] - Rb[0] - Rb[8]) * 2.f;
    qq[3] = (Rb[2] - Rb[6]) / sc; qq[0] = (Rb[1] + Rb[3]) / sc; qq[1] = 0.25f * sc; qq[2] = (Rb[5] + Rb[7]) / sc;
  } else {
    const float sc = sqrtf(1.f + Rb[8] - Rb[0] - Rb[4]) * 2.f;
    qq[3] = (Rb[3] - Rb[1]) / sc; qq[0] = (Rb[2] + Rb[6]) / sc; qq[1] = (Rb[5] + Rb[7]) / sc; qq[2] = 0.25f * sc;
  }
  if (qq[3] < 0.f)
    for (int i = 0; i < 4; ++i) qq[i] = -qq[i];
}

// ------------------------------------------------------------------ one env step
// legged_robot.py:67-100 (+ Go2Robot.post_physics_step go2.py:345-387 / LeggedRobot
// legged_robot.py:103-138) for env e; `stats` receives its episode statistics when it resets.
static void env_step(Env& s, const lgx_model* M, const lgx_task_params* P, const lgx_buffers* B, uint64_t seed,
                     uint64_t step, bool physics, int e, float* stats) {
  const int D = P->num_dof, A = P->num_actions, NB = P->num_bodies, F = P->num_feet;
  const bool go2 = P->task_kind == LGX_TASK_GO2;
  float* root_g = B->root_states + (size_t)e * 13;
  for (int j = 0; j < A; ++j) {  // clip actions legged_robot.py:74-75
    const float a = clipf(B->actions_in[(size_t)e * A + j], -P->clip_actions, P->clip_actions);
    s.act[j] = a;
    B->actions[(size_t)e * A + j] = a;
  }
  for (int j = 0; j < D; ++j) {
    s.th[j] = B->dof_state[((size_t)e * D + j) * 2];
    s.thd[j] = B->dof_state[((size_t)e * D + j) * 2 + 1];
    s.kpm[j] = B->kp_kd ? B->kp_kd[(size_t)e * D + j] : 1.f;
    s.kdm[j] = B->kp_kd ? B->kp_kd[((size_t)P->num_envs + e) * D + j] : 1.f;
    s.ldv[j] = B->last_dof_vel[(size_t)e * D + j];
  }
  memcpy(s.root, root_g, sizeof(s.root));
  s.madd = B->mass_params ? B->mass_params[e * 4] : 0.f;
  for (int i = 0; i < 3; ++i) s.cadd[i] = B->mass_params ? B->mass_params[e * 4 + 1 + i] : 0.f;
  s.mu = 0.5f * ((B->friction ? B->friction[e] : 1.f) + P->ground_friction);
  memcpy(s.cmd, B->commands + e * 4, sizeof(s.cmd));
  const long long ep_prev = B->episode_length[e];
  const float jump_prev = B->rpy_phase ? B->rpy_phase[e * 8 + 7] : 0.f;
  int blew = 0;  // NaN/Inf guard

  if (physics) {
    const float* r0 = s.root;
    const float nq = 1.0f / sqrtf(r0[3] * r0[3] + r0[4] * r0[4] + r0[5] * r0[5] + r0[6] * r0[6]);
    for (int i = 0; i < 4; ++i) s.qb[i] = r0[3 + i] * nq;
    for (int i = 0; i < 3; ++i) { s.pb[i] = r0[i]; s.wb[i] = r0[10 + i]; }
    float R[9];
    quat_to_R(s.qb, R);
    const f3 rc = mv(R, mk(M->link_com[0][0] + s.cadd[0], M->link_com[0][1] + s.cadd[1], M->link_com[0][2] + s.cadd[2]));
    st3(s.vo, ld3(r0 + 7) - cross(ld3(s.wb), rc));  // COM velocity -> origin velocity
    // external force (include/lgx.h, ABI 16): the kernel's rule
    s.fon = 0;
    if (B->force_window) {
      const int32_t* fwin = B->force_window + (size_t)e * 3;
      const float* fv = B->force_vec + (size_t)e * 6;
      if (force_window_on(fwin[0], fwin[1], fwin[2], ep_prev + 1) && (fv[0] != 0.f || fv[1] != 0.f || fv[2] != 0.f)) {
        s.fon = 1;
        force_to_world(r0 + 3, fv, s.fw);
        for (int i = 0; i < 3; ++i) s.fpt[i] = fv[3 + i];
      }
    }
    for (int sub = 0; sub < P->decimation; ++sub) substep(s, M, P, B, e, sub, sub == P->decimation - 1);
    // NaN/Inf guard (the kernel's rule, lgx_env.hip): a non-finite state after the substeps
    // becomes a finite stand-in and the env is reset below
    bool bad = false;
    for (int j = 0; j < D; ++j) bad = bad || !(std::isfinite(s.th[j]) && std::isfinite(s.thd[j]) && std::isfinite(s.tau[j]));
    for (int j = 0; j < A; ++j) bad = bad || !std::isfinite(s.act[j]);
    for (int i = 0; i < 3; ++i) bad = bad || !(std::isfinite(s.pb[i]) && std::isfinite(s.vo[i]) && std::isfinite(s.wb[i]));
    for (int i = 0; i < 4; ++i) bad = bad || !std::isfinite(s.qb[i]);
    for (int b = 0; b < NB; ++b)
      for (int i = 0; i < 3; ++i) bad = bad || !std::isfinite(s.cf[b][i]);
    if (bad) {
      for (int j = 0; j < D; ++j) { s.th[j] = P->default_dof_pos[j]; s.thd[j] = 0.f; s.tau[j] = 0.f; }
      for (int j = 0; j < A; ++j) { s.act[j] = 0.f; B->actions[(size_t)e * A + j] = 0.f; }
      for (int i = 0; i < 3; ++i) { s.pb[i] = std::isfinite(s.root[i]) ? s.root[i] : 0.f; s.vo[i] = 0.f; s.wb[i] = 0.f; }
      for (int i = 0; i < 4; ++i) s.qb[i] = i == 3 ? 1.f : 0.f;
      for (int b = 0; b < NB; ++b) s.cf[b][0] = s.cf[b][1] = s.cf[b][2] = 0.f;
      blew = 1;
    }
    kinematics<false>(s, M, P);
    quat_to_R(s.qb, R);
    const f3 rc2 = mv(R, mk(M->link_com[0][0] + s.cadd[0], M->link_com[0][1] + s.cadd[1], M->link_com[0][2] + s.cadd[2]));
    const f3 vc = ld3(s.vo) + cross(ld3(s.wb), rc2);
    float* root = s.root;
    for (int i = 0; i < 3; ++i) root[i] = s.pb[i];
    for (int i = 0; i < 4; ++i) root[3 + i] = s.qb[i];
    root[7] = vc.x; root[8] = vc.y; root[9] = vc.z;
    for (int i = 0; i < 3; ++i) root[10 + i] = s.wb[i];
    for (int b = 0; b < NB; ++b) {
      const Link& lk = s.lk[M->body_link[b]];
      const f3 off = ld3(M->body_offset[b]), o = mv(lk.R, off), pos = ld3(lk.P) + o;
      const bool primary = off.x == 0.f && off.y == 0.f && off.z == 0.f;
      const f3 lv = ld3(lk.V) + cross(ld3(lk.W), primary ? (ld3(lk.C) - ld3(lk.P)) : o);
      float Rb[9], qq[4];
      mm(lk.R, M->body_rot[b], Rb);
      mat_quat(Rb, qq);
      float* rb = B->rigid_body_states + ((size_t)e * NB + b) * 13;
      rb[0] = pos.x; rb[1] = pos.y; rb[2] = pos.z;
      for (int i = 0; i < 4; ++i) rb[3 + i] = qq[i];
      rb[7] = lv.x; rb[8] = lv.y; rb[9] = lv.z;
      for (int i = 0; i < 3; ++i) rb[10 + i] = lk.W[i];
      s.rbz[b] = pos.z;
      memcpy(B->contact_forces + ((size_t)e * NB + b) * 3, s.cf[b], sizeof(float) * 3);
    }
    memcpy(B->torques + (size_t)e * D, s.tau, sizeof(float) * D);
  } else {  // post-physics only: physics state supplied by the caller
    for (int b = 0; b < NB; ++b) {
      memcpy(s.cf[b], B->contact_forces + ((size_t)e * NB + b) * 3, sizeof(float) * 3);
      s.rbz[b] = B->rigid_body_states[((size_t)e * NB + b) * 13 + 2];
    }
    memcpy(s.tau, B->torques + (size_t)e * D, sizeof(float) * D);
  }

  // ---------------------------------------------------------------- post-physics
  fill_uniforms(s, P, seed, (uint32_t)(P->env_id_offset + e), step, 0);
  float* root = s.root;
  float* cmd = s.cmd;
  const long long ep = ep_prev + 1;
  s.ep = ep;
  const float g[3] = {0.f, 0.f, -1.f};
  quat_rotate_inverse(root + 3, root + 7, s.x.blv);
  quat_rotate_inverse(root + 3, root + 10, s.x.bav);
  quat_rotate_inverse(root + 3, g, s.x.pg);
  s.x.roll = s.x.pitch = s.x.yaw = 0.f;
  for (int f = 0; f < 4; ++f) { s.x.ph[f] = 0.f; s.x.contact[f] = 0; s.x.feet_z[f] = 0.f; s.lc[f] = 0; s.lch[f] = 0.f; s.fat[f] = 0.f; }
  if (go2) {  // update_feet_states go2.py:266-328
    const float phase = trem((float)ep * P->dt, P->period) / P->period;
    const float pfr = trem(phase + P->offset_fr, 1.0f), pbl = trem(phase + P->offset_bl, 1.0f);
    const float pfl = trem(phase + P->offset_fl, 1.0f), pbr = trem(phase + P->offset_br, 1.0f);
    const float msk = (nrm3(cmd[0], cmd[1], cmd[2]) < 0.2f) ? 0.0f : 1.0f;
    s.x.ph[0] = pfl * msk; s.x.ph[1] = pfr * msk; s.x.ph[2] = pbl * msk; s.x.ph[3] = pbr * msk;
    for (int f = 0; f < F; ++f) {
      const int lcf = B->last_contacts[e * F + f];
      const float lch = B->last_contact_heights[e * F + f];
      const int curc = s.cf[P->feet_idx[f]][2] > 1.0f;
      s.x.contact[f] = curc || lcf;
      s.lc[f] = curc;
      s.x.feet_z[f] = s.rbz[P->feet_idx[f]];
      s.lch[f] = s.x.contact[f] ? s.x.feet_z[f] : lch;
      if (B->feet_air_time) s.fat[f] = B->feet_air_time[e * F + f];
    }
    const float qx = root[3], qy = root[4], qz = root[5], qw = root[6];  // go2.py:11-31
    s.x.roll = atan2f(2.0f * (qw * qx + qy * qz), 1.0f - 2.0f * (qx * qx + qy * qy));
    s.x.pitch = asinf(clipf(2.0f * (qw * qy - qz * qx), -1.0f, 1.0f));
    s.x.yaw = atan2f(2.0f * (qw * qz + qx * qy), 1.0f - 2.0f * (qy * qy + qz * qz));
  }
  // _post_physics_step_callback go2.py:390-410
  if (ep % P->resample_interval == 0) resample_commands(P, B->command_ranges, cmd, s.U, S_CMD, root + 3);
  if (P->heading_command) {
    const float fwd[3] = {1.f, 0.f, 0.f};
    float f[3];
    quat_apply(root + 3, fwd, f);
    cmd[2] = clipf(wrap_to_pi(cmd[3] - atan2f(f[1], f[0])) * (go2 ? P->heading_error_gain : 0.5f), -1.0f, 1.0f);
  }
  // command schedule (include/lgx.h, ABI 10): after the resample and the heading rule
  if (B->cmd_step)
    scheduled_command(cmd, B->cmd_step + (size_t)e * LGX_CMD_SEGMENTS,
                      B->cmd_val + (size_t)e * LGX_CMD_SEGMENTS * 4, ep);
  if (P->push_robots && (step % (uint64_t)P->push_interval == 0)) {
    root[7] = rand_range(-P->max_push_vel_xy, P->max_push_vel_xy, s.U[S_PUSH + 0]);
    root[8] = rand_range(-P->max_push_vel_xy, P->max_push_vel_xy, s.U[S_PUSH + 1]);
  }
  // scheduled push (include/lgx.h, ABI 9): ep >= 1, so a push_step <= 0 never fires
  if (B->push_step && (long long)B->push_step[e] == ep) scheduled_push(root, B->push_dvel + (size_t)e * 3);
  // check_termination go2.py:186-204
  int reset = 0;
  for (int i = 0; i < P->n_termination; ++i) reset |= fnorm(s.cf[P->termination_idx[i]]) > 1.0f;
  const int tout = ep > P->max_episode_length && !blew;  // a blow-up is a termination (kernel)
  reset |= tout;
  reset |= s.x.pg[2] > 0.0f;
  if (P->parkour) reset |= root[2] < -1.0f;
  reset |= blew;
  s.x.jump = jump_prev;
  get_heights(P, B, s);
  joint_sums(P, B, s, e);
  // compute_reward legged_robot.py:216-237: the terms in the reference's (alphabetical) order
  const int K = P->num_reward_terms, KS = K + (P->has_termination_reward ? 1 : 0);
  float rew = 0.0f;
  for (int k = 0; k < K; ++k) {
    s.rterm[k] = blew ? 0.0f : reward_term(P, s, P->reward_ids[k]) * P->reward_scales[k];
  }
  for (int k = 0; k < K; ++k) rew += s.rterm[k];
  if (P->only_positive_rewards) rew = rew < 0.0f ? 0.0f : rew;
  if (P->has_termination_reward) {
    const float v = (float)(reset && !tout && !blew) * P->termination_scale;
    rew += v;
    s.rterm[K] = v;
  }
  B->rew[e] = rew;
  B->reset[e] = (uint8_t)reset;
  B->time_out[e] = (uint8_t)tout;
  if (B->blew_up) B->blew_up[e] = (uint8_t)blew;
  if (blew && B->blowup_count) {
#pragma omp atomic
    *B->blowup_count += 1u;
  }
  for (int k = 0; k < KS; ++k) B->episode_sums[(size_t)e * KS + k] += s.rterm[k];
  // scan model (include/lgx.h, ABI 17): the second lookup uses the pose the height scan used
  const float scan_pose[4] = {s.root[0], s.root[1], s.root[5], s.root[6]};
  if (reset) reset_env(P, B, s, e, false, stats);  // reset_idx go2.py:207-263

  // compute_observations go2.py:467-574 / legged_robot.py:240-273
  const int Pp = P->num_proprio, H = P->history_len;
  if (go2 && P->parkour) {
    int outl = 0;
    for (int i = 0; i < P->num_height_points; ++i) outl += fabsf(s.heights[i]) > 0.1f;
    s.x.jump = (float)(outl >= 8);
  }
  int sens_c = 0, sens_d = 0;  // sensor model: this episode's rows in the ring, the clamped latency
  if (B->sensor_count) {
    sens_c = reset ? 0 : B->sensor_count[e];
    if (B->obs_delay) sens_d = sensor_delay_clamp(B->obs_delay[e], P->sensor_history_len, sens_c);
  }
  for (int i = 0; i < Pp; ++i) {
    float v;
    if (go2) {
      if (i < 3) v = s.x.bav[i] * P->obs_scale_ang_vel;
      else if (i == 3) v = s.x.roll;
      else if (i == 4) v = s.x.pitch;
      else if (i < 8) v = s.cmd[i - 5] * P->commands_scale[i - 5];
      else if (i < 8 + D) v = (s.th[i - 8] - P->default_dof_pos[i - 8]) * P->obs_scale_dof_pos;
      else if (i < 8 + 2 * D) v = s.thd[i - 8 - D] * P->obs_scale_dof_vel;
      else if (i < 8 + 2 * D + A) v = s.act[i - 8 - 2 * D];
      else {
        const int q = i - (8 + 2 * D + A);  // sin/cos of FR, FL, BL, BR
        const int leg = (q >> 1) == 0 ? 1 : ((q >> 1) == 1 ? 0 : (q >> 1));
        const float p = 6.283185307179586f * s.x.ph[leg];
        v = (q & 1) ? cosf(p) : sinf(p);
      }
    } else {
      if (i < 3) v = s.x.blv[i] * P->obs_scale_lin_vel;
      else if (i < 6) v = s.x.bav[i - 3] * P->obs_scale_ang_vel;
      else if (i < 9) v = s.x.pg[i - 6];
      else if (i < 12) v = s.cmd[i - 9] * P->commands_scale[i - 9];
      else if (i < 12 + D) v = (s.th[i - 12] - P->default_dof_pos[i - 12]) * P->obs_scale_dof_pos;
      else if (i < 12 + 2 * D) v = s.thd[i - 12 - D] * P->obs_scale_dof_vel;
      else if (i < 12 + 2 * D + A) v = s.act[i - 12 - 2 * D];
      else v = clipf(s.root[2] - 0.5f - s.heights[i - (12 + 2 * D + A)], -1.0f, 1.0f) * P->obs_scale_height;
    }
    // sensor model (include/lgx.h, ABI 15): the kernel's rule
    if (B->sensor_history) {
      const int SK = P->sensor_history_len;
      float* ring = B->sensor_history + (size_t)e * SK * Pp;
      const float raw = v;
      if (sens_d > 0 && sensor_channel(go2, i, D, A)) v = ring[(size_t)sensor_ring_read_row(sens_c, sens_d, SK) * Pp + i];
      ring[(size_t)sensor_ring_write_row(sens_c, SK) * Pp + i] = raw;
    }
    v = sensor_noise_bias(v, P->add_noise != 0, P->add_noise ? s.U[S_NOISE + i] : 0.f, P->noise_vec[i],
                          B->obs_noise_scale ? B->obs_noise_scale + e : nullptr,
                          B->obs_bias ? B->obs_bias + (size_t)e * Pp + i : nullptr);
    s.cur[i] = v;
  }
  if (B->sensor_count) B->sensor_count[e] = sens_c + 1;
  float* hist_g = B->obs_history + (size_t)e * H * Pp;
  for (int i = 0; i < H * Pp; ++i) s.hist[i] = reset ? 0.f : hist_g[i];  // go2.py:238
  const float co = P->clip_obs;
  float* obs = B->obs + (size_t)e * P->num_obs;
  float* cr = B->critic ? B->critic + (size_t)e * P->num_critic : nullptr;
  for (int i = 0; i < H * Pp; ++i) {
    const float v = clipf(s.hist[i], -co, co);
    obs[i] = v;
    if (go2 && cr) cr[i] = v;
  }
  for (int i = 0; i < Pp; ++i) {
    const float v = clipf(s.cur[i], -co, co);
    obs[H * Pp + i] = v;
    if (go2 && cr) cr[H * Pp + i] = v;
  }
  if (go2) {
    const int NO = P->num_obs;
    for (int i = 0; i < P->num_priv; ++i) {  // [mass params (4), friction, kp-1 (D), kd-1 (D)]
      float v;
      if (i < 4) v = B->mass_params[e * 4 + i];
      else if (i == 4) v = B->friction[e];
      else if (i < 5 + D) v = s.kpm[i - 5] - 1.0f;
      else v = s.kdm[i - 5 - D] - 1.0f;
      v = clipf(v, -co, co);
      B->priv[(size_t)e * P->num_priv + i] = v;
      if (cr) cr[NO + i] = v;
    }
    for (int i = 0; i < 3; ++i) {
      const float v = clipf(s.x.blv[i] * P->obs_scale_lin_vel, -co, co);
      B->est[(size_t)e * P->num_est + i] = v;
      if (cr) cr[NO + P->num_priv + i] = v;
    }
    // height-scan model (include/lgx.h, ABI 17): the kernel's rule; all unbound = the clean scan
    const int S = P->num_scan, SK = P->sensor_history_len;
    const uint32_t gid = (uint32_t)(P->env_id_offset + e);
    const float amp = B->scan_noise ? B->scan_noise[e] : 0.f;
    const float drop_p = B->scan_dropout ? B->scan_dropout[(size_t)e * 2] : 0.f;
    const float fill = B->scan_dropout ? B->scan_dropout[(size_t)e * 2 + 1] : 0.f;
    const float* off = B->scan_offset ? B->scan_offset + (size_t)e * 3 : nullptr;
    const float dx = off ? off[0] : 0.f, dy = off ? off[1] : 0.f, dz = off ? off[2] : 0.f;
    const bool second = (dx != 0.f || dy != 0.f) && P->mesh_type != LGX_MESH_PLANE && B->height_samples != nullptr;
    float qy[4] = {0.f, 0.f, 0.f, 1.f};
    if (second) scan_yaw_quat(scan_pose[2], scan_pose[3], qy);
    const int scan_d = B->scan_delay ? sensor_delay_clamp(B->scan_delay[e], SK, sens_c) : 0;
    for (int i = 0; i < S; ++i) {
      const float clean = scan_raw(s.root[2], s.heights[i]);
      float raw = clean;
      if (second)
        raw = scan_raw(s.root[2], scan_point_height(P, B->height_samples, qy, scan_pose,
                                                    P->height_points[i][0] + dx, P->height_points[i][1] + dy));
      float v = raw;
      if (B->scan_history) {
        float* ring = B->scan_history + (size_t)e * SK * S;
        if (scan_d > 0) v = ring[(size_t)sensor_ring_read_row(sens_c, scan_d, SK) * S + i];
        ring[(size_t)sensor_ring_write_row(sens_c, SK) * S + i] = raw;
      }
      const float u = amp != 0.f ? scan_uniform(seed, gid, step, i) : 0.f;
      const float ud = drop_p > 0.f ? scan_uniform(seed, gid, step, LGX_MAX_HEIGHT_POINTS + i) : 0.f;
      B->scan[(size_t)e * S + i] = scan_point_model(v, amp, u, dz, drop_p, ud, fill);
      if (cr) cr[NO + P->num_priv + 3 + i] = clipf(clean, -co, co);
    }
  }
  for (int i = 0; i < H * Pp; ++i)  // history update go2.py:570-574
    hist_g[i] = (s.ep <= 1) ? s.cur[i % Pp] : (i < (H - 1) * Pp ? s.hist[i + Pp] : s.cur[i - (H - 1) * Pp]);
  // last_* copies go2.py:380-384 and state write-back
  memcpy(B->last_actions + (size_t)e * A, s.act, sizeof(float) * A);
  if (B->action_history)
    for (int j = 0; j < A; ++j)
      action_history_push(B->action_history + (size_t)e * P->action_history_len * A, P->action_history_len, A, j,
                          s.act[j], reset != 0);
  for (int j = 0; j < D; ++j) {
    B->last_dof_vel[(size_t)e * D + j] = s.thd[j];
    B->last_torques[(size_t)e * D + j] = s.tau[j];
    B->dof_state[((size_t)e * D + j) * 2] = s.th[j];
    B->dof_state[((size_t)e * D + j) * 2 + 1] = s.thd[j];
  }
  memcpy(B->last_root_vel + e * 6, s.root + 7, sizeof(float) * 6);
  memcpy(B->last_base_lin_vel + e * 3, s.x.blv, sizeof(float) * 3);
  if (B->base_lin_vel) memcpy(B->base_lin_vel + e * 3, s.x.blv, sizeof(float) * 3);
  if (B->base_ang_vel) memcpy(B->base_ang_vel + e * 3, s.x.bav, sizeof(float) * 3);
  if (B->projected_gravity) memcpy(B->projected_gravity + e * 3, s.x.pg, sizeof(float) * 3);
  memcpy(root_g, s.root, sizeof(float) * 13);
  memcpy(B->commands + e * 4, s.cmd, sizeof(float) * 4);
  if (go2 && !reset)
    for (int f = 0; f < F; ++f) {
      B->last_contacts[e * F + f] = (uint8_t)s.lc[f];
      B->last_contact_heights[e * F + f] = s.lch[f];
      if (B->feet_air_time) B->feet_air_time[e * F + f] = s.fat[f];
    }
  B->episode_length[e] = s.ep;
  if (B->rpy_phase) {
    const float v[8] = {s.x.roll, s.x.pitch, s.x.yaw, s.x.ph[0], s.x.ph[1], s.x.ph[2], s.x.ph[3], s.x.jump};
    memcpy(B->rpy_phase + e * 8, v, sizeof(v));
  }
  if (B->measured_heights)
    memcpy(B->measured_heights + (size_t)e * P->num_height_points, s.heights, sizeof(float) * P->num_height_points);
}

// Episode statistics (extras['episode'] numerators and the reset count): per-env rows of
// the envs that reset, summed in env order after the parallel loop (deterministic).
static void fold_stats(const lgx_buffers* B, int N, int KS, const std::vector<float>& rows,
                       const std::vector<uint8_t>& hit) {
  if (!B->episode_stats) return;
  for (int e = 0; e < N; ++e)
    if (hit[e])
      for (int k = 0; k <= KS; ++k) B->episode_stats[k] += rows[(size_t)e * (KS + 1) + k];
}

void step(const lgx_model* M, const lgx_task_params* P, const lgx_buffers* B, uint64_t seed, uint64_t stepn,
          bool physics) {
  const int N = P->num_envs, KS = P->num_reward_terms + (P->has_termination_reward ? 1 : 0);
  std::vector<float> rows((size_t)N * (KS + 1), 0.f);
  std::vector<uint8_t> hit(N, 0);
#pragma omp parallel
  {
    Env* s = new Env;
#pragma omp for schedule(dynamic, 4)
    for (int e = 0; e < N; ++e) {
      env_step(*s, M, P, B, seed, stepn, physics, e, &rows[(size_t)e * (KS + 1)]);
      hit[e] = B->reset[e];
    }
    delete s;
  }
  fold_stats(B, N, KS, rows, hit);
}

void reset(const lgx_task_params* P, const lgx_buffers* B, const uint8_t* mask, uint64_t seed, uint64_t call) {
  const int N = P->num_envs, D = P->num_dof, KS = P->num_reward_terms + (P->has_termination_reward ? 1 : 0);
  std::vector<float> rows((size_t)N * (KS + 1), 0.f);
  std::vector<uint8_t> hit(mask, mask + N);
#pragma omp parallel
  {
    Env* s = new Env;
#pragma omp for schedule(static)
    for (int e = 0; e < N; ++e) {
      if (!mask[e]) continue;
      fill_uniforms(*s, P, seed, (uint32_t)(P->env_id_offset + e), call, 1);
      memcpy(s->root, B->root_states + (size_t)e * 13, sizeof(s->root));
      memcpy(s->cmd, B->commands + e * 4, sizeof(s->cmd));
      // an external reset exists only once the env is built: the terrain curriculum applies
      reset_env(P, B, *s, e, true, &rows[(size_t)e * (KS + 1)]);
      memcpy(B->root_states + (size_t)e * 13, s->root, sizeof(s->root));
      for (int j = 0; j < D; ++j) {
        B->dof_state[((size_t)e * D + j) * 2] = s->th[j];
        B->dof_state[((size_t)e * D + j) * 2 + 1] = s->thd[j];
      }
      memcpy(B->commands + e * 4, s->cmd, sizeof(s->cmd));
      B->episode_length[e] = s->ep;
      B->reset[e] = 1;
    }
    delete s;
  }
  fold_stats(B, N, KS, rows, hit);
}

void episode_extras(const lgx_task_params* P, const lgx_buffers* B, float* means, float* level_mean,
                    uint8_t* time_outs, uint64_t* step_counter) {
  const int N = P->num_envs, KS = P->num_reward_terms + (P->has_termination_reward ? 1 : 0);
  float* st = B->episode_stats;
  const float cnt = st[KS];
  const float inv_T = 1.0f / P->max_episode_length_s;  // torch: tensor / python float
  if (cnt > 0.f) {
    for (int k = 0; k < KS; ++k) means[k] = st[k] / cnt * inv_T;
    if (level_mean) {
      double t = 0.0;
      for (int e = 0; e < N; ++e) t += (double)B->terrain_levels[e];
      *level_mean = (float)(t / N);
    }
  }
  if (time_outs) {
    int any = 0;
    for (int e = 0; e < N && !any; ++e) any |= B->reset[e];
    if (any) memcpy(time_outs, B->time_out, (size_t)N);
  }
  for (int k = 0; k <= KS; ++k) st[k] = 0.f;
  if (step_counter) *step_counter += 1;
}

// update_command_curriculum (go2.py:80-107 / legged_robot.py:580-591): the kernel's rule
// (lgx_env.hip curriculum_kernel), envs in order
void command_curriculum(const lgx_task_params* P, const lgx_buffers* B, uint64_t seed, uint64_t step,
                        const double* global_sum_count) {
  if (step % (uint64_t)P->max_episode_length != 0) return;
  const int N = P->num_envs;
  double S = 0.0, Cn = 0.0;
  if (global_sum_count) {
    S = global_sum_count[0];
    Cn = global_sum_count[1];
  } else {
    for (int e = 0; e < N; ++e)
      if (B->reset[e]) { S += (double)B->curriculum_vals[e]; Cn += 1.0; }
  }
  if (!curriculum_update_ranges(P, *B, S, Cn)) return;
  for (int e = 0; e < N; ++e)
    if (B->reset[e]) curriculum_rewrite_env(P, *B, seed, step, e);
}

void eval_begin(const lgx_task_params* P, const lgx_eval_buffers* E) {
  const size_t N = (size_t)P->num_envs;
  memset(E->acc, 0, sizeof(float) * LGX_EVAL_METRICS * N);
  memset(E->status, 0, N);
  if (E->overflow) *E->overflow = 0;
  if (E->push_rec) memset(E->push_rec, 0, sizeof(float) * LGX_EVAL_PUSH_REC * N);
  if (E->cmd_rec) memset(E->cmd_rec, 0, sizeof(float) * LGX_EVAL_CMD_REC * N);
}

// lgx_eval_accumulate (include/lgx.h): the kernel's arithmetic (lgx_env.hip
// eval_accumulate_kernel), the joint sums in joint order
void eval_accumulate(const lgx_task_params* P, const lgx_buffers* B, const lgx_eval_buffers* E) {
  const int N = P->num_envs, D = P->num_dof, NB = P->num_bodies;
  const float dt = P->dt;
#pragma omp parallel for schedule(static)
  for (int e = 0; e < N; ++e) {
    if (E->status[e] != 0) continue;
    if (B->reset[e]) {
      E->status[e] = episode_end_status(*B, e);
      continue;
    }
    const float* v = B->base_lin_vel + (size_t)e * 3;
    const float* w = B->base_ang_vel + (size_t)e * 3;
    const float* c = B->commands + (size_t)e * 4;
    const float* tq = B->torques + (size_t)e * D;
    const float* ds = B->dof_state + (size_t)e * D * 2;
    float en = 0.f, t2 = 0.f, fm = 0.f;
    for (int j = 0; j < D; ++j) {
      en += fabsf(tq[j] * ds[2 * j + 1]);
      t2 += tq[j] * tq[j];
    }
    for (int f = 0; f < P->num_feet; ++f) {
      const float* cf = B->contact_forces + ((size_t)e * NB + P->feet_idx[f]) * 3;
      fm = std::max(fm, sqrtf(cf[0] * cf[0] + cf[1] * cf[1] + cf[2] * cf[2]));
    }
    float* a = E->acc + (size_t)e * LGX_EVAL_METRICS;
    a[0] += 1.0f;
    a[1] += (c[0] - v[0]) * (c[0] - v[0]) + (c[1] - v[1]) * (c[1] - v[1]);
    a[2] += (c[2] - w[2]) * (c[2] - w[2]);
    a[3] += v[0] * dt;
    a[4] += sqrtf(v[0] * v[0] + v[1] * v[1]) * dt;
    a[5] += dt * en;
    a[6] += t2;
    a[7] = std::max(a[7], fm);
    if (E->push_rec) {  // push recovery (ABI 9)
      const int ps = B->push_step[e];
      const long long k = (long long)B->episode_length[e] - ps;
      if (ps > 0 && k > 0) {
        float* r = E->push_rec + (size_t)e * LGX_EVAL_PUSH_REC;
        for (int col = 0; col < LGX_EVAL_PUSH_REC; ++col)
          r[col] = push_record_col(col, r[col], B->projected_gravity + (size_t)e * 3, c, v, k, E->settle_tol);
      }
    }
    if (E->cmd_rec) {  // step response (ABI 10)
      const int sw = E->cmd_switch_step[e];
      const long long k = (long long)B->episode_length[e] - sw;
      if (sw > 0 && k >= 0) {
        float* r = E->cmd_rec + (size_t)e * LGX_EVAL_CMD_REC;
        for (int col = 0; col < LGX_EVAL_CMD_REC; ++col)
          r[col] = command_record_col(col, r[col], B->projected_gravity + (size_t)e * 3, c, v, w, k, E->settle_tol,
                                      E->yaw_tol, E->steady_after);
      }
    }
  }
}

// The start of eval_reduce / gait_reduce: counts the envs outside the rows x cols grid, publishes
// the count and returns it; when it is 0, zeroes the cell tables (pointer, columns per cell; a NULL
// one is skipped), which the caller then fills in env order.
struct CellTable { double* cells; int cols; };
static int reduce_begin(const lgx_buffers* B, const int32_t* cell_ids, int N, int rows, int cols, uint32_t* overflow,
                        std::initializer_list<CellTable> tables) {
  int bad = 0;
  for (int e = 0; e < N; ++e) bad += cell_of_env(B->terrain_levels, B->terrain_types, cell_ids, e, rows, cols) < 0;
  *overflow = (uint32_t)bad;
  if (bad) return bad;
  for (const CellTable& t : tables)
    if (t.cells) std::fill(t.cells, t.cells + (size_t)rows * cols * t.cols, 0.0);
  return 0;
}

int eval_reduce(const lgx_task_params* P, const lgx_buffers* B, const lgx_eval_buffers* E) {
  const int N = P->num_envs, rows = E->cell_rows, cols = E->cell_cols;
  if (int bad = reduce_begin(B, E->cell_ids, N, rows, cols, E->overflow,
                             {{E->cells, LGX_EVAL_CELL_COLS}, {E->push_cells, LGX_EVAL_PUSH_COLS},
                              {E->cmd_cells, LGX_EVAL_CMD_COLS}}))
    return bad;
  for (int e = 0; e < N; ++e) {  // env order: deterministic
    const size_t id = (size_t)cell_of_env(B->terrain_levels, B->terrain_types, E->cell_ids, e, rows, cols);
    double* cl = E->cells + id * LGX_EVAL_CELL_COLS;
    const int st = E->status[e];
    cl[0] += 1.0;
    if (st == 0) continue;
    if (st >= 1 && st <= 3) cl[st] += 1.0;
    const float* a = E->acc + (size_t)e * LGX_EVAL_METRICS;
    for (int k = 0; k < LGX_EVAL_METRICS; ++k) cl[4 + k] += (double)a[k];
    const float* r = E->push_cells ? E->push_rec + (size_t)e * LGX_EVAL_PUSH_REC : nullptr;
    if (r && r[0] > 0.f) {
      double* pc = E->push_cells + id * LGX_EVAL_PUSH_COLS;
      pc[0] += 1.0;
      pc[1] += (double)r[1];
      pc[2] += (double)r[2];
      if (st == 1) { pc[3] += 1.0; pc[4] += (double)r[3]; }
    }
    const float* cr = E->cmd_cells ? E->cmd_rec + (size_t)e * LGX_EVAL_CMD_REC : nullptr;
    if (cr && cr[0] > 0.f) {
      double* cc = E->cmd_cells + id * LGX_EVAL_CMD_COLS;
      cc[0] += 1.0;
      cc[4] += (double)cr[3];
      if (st == 1) {
        cc[1] += 1.0;
        cc[2] += (double)cr[1];
        cc[3] += (double)cr[2];
        for (int k = 4; k < LGX_EVAL_CMD_REC; ++k) cc[1 + k] += (double)cr[k];
      }
    }
  }
  return 0;
}

// The start of a per-step record (trace, gait, joint) for env e: false when the env is frozen
// (status != 0), or when it is reset in this step, which latches episode_end_status and takes no
// sample.
static bool still_recording(uint8_t* status, const lgx_buffers& B, int e) {
  if (status[e] != 0) return false;
  if (B.reset[e]) {
    status[e] = episode_end_status(B, e);
    return false;
  }
  return true;
}

// The *_begin of the records that start all zero: two per-env arrays of na and nb 4-byte entries per
// env, the statuses and, for a record with cells, the overflow count.
static void zero_records(void* a, size_t na, void* b, size_t nb, uint8_t* status, uint32_t* overflow, size_t N) {
  static_assert(sizeof(float) == 4 && sizeof(int32_t) == 4, "4-byte entries");
  memset(a, 0, 4 * na * N);
  memset(b, 0, 4 * nb * N);
  memset(status, 0, N);
  if (overflow) *overflow = 0;
}

void trace_begin(const lgx_task_params* P, const lgx_trace_buffers* T) {
  zero_records(T->ring, LGX_TRACE_COLS * (size_t)T->depth, T->count, 1, T->status, nullptr, (size_t)P->num_envs);
}

// lgx_trace_record (include/lgx.h): the kernel's arithmetic (lgx_env.hip trace_record_kernel), the
// columns and the bodies in order
void trace_record(const lgx_task_params* P, const lgx_buffers* B, const lgx_trace_buffers* T) {
  const int N = P->num_envs, NB = P->num_bodies, depth = T->depth;
#pragma omp parallel for schedule(static)
  for (int e = 0; e < N; ++e) {
    if (!still_recording(T->status, *B, e)) continue;
    const int cnt = T->count[e];
    float* dst = T->ring + ((size_t)e * depth + (size_t)(cnt % depth)) * LGX_TRACE_COLS;
    for (int col = 0; col < 74; ++col) dst[col] = trace_col(col, P, *B, e);
    float pn = 0.f;
    int pb = -1;
    for (int b = 0; b < NB; ++b) {
      if (trace_is_foot(P, b)) continue;
      const float* c = B->contact_forces + ((size_t)e * NB + b) * 3;
      trace_peak_merge(pn, pb, nrm3(c[0], c[1], c[2]), b);
    }
    dst[74] = pn;
    dst[75] = (float)pb;
    T->count[e] = cnt + 1;
  }
}

void trace_gather(const lgx_task_params* P, const lgx_trace_buffers* T, const int32_t* ids, int32_t m, float* out,
                  int32_t* out_len) {
  const int N = P->num_envs, depth = T->depth;
  const size_t per = (size_t)depth * LGX_TRACE_COLS;
#pragma omp parallel for schedule(static)
  for (int i = 0; i < m; ++i) {
    float* o = out + (size_t)i * per;
    memset(o, 0, sizeof(float) * per);
    const int e = ids[i];
    if (e < 0 || e >= N) {
      out_len[i] = -1;
      continue;
    }
    const int cn = T->count[e], L = std::max(0, std::min(cn, depth));
    for (int j = 0; j < L; ++j)
      memcpy(o + (size_t)(depth - L + j) * LGX_TRACE_COLS,
             T->ring + ((size_t)e * depth + (size_t)((cn - L + j) % depth)) * LGX_TRACE_COLS,
             sizeof(float) * LGX_TRACE_COLS);
    out_len[i] = L;
  }
}

void gait_begin(const lgx_task_params* P, const lgx_gait_buffers* G) {
  zero_records(G->foot, LGX_GAIT_FOOT_COLS * LGX_MAX_FEET, G->body, LGX_GAIT_BODY_COLS, G->status, G->overflow,
               (size_t)P->num_envs);
}

// lgx_gait_record (include/lgx.h): the kernel's arithmetic (lgx_env.hip gait_record_kernel), the
// feet and the body columns in order
void gait_record(const lgx_task_params* P, const lgx_buffers* B, const lgx_gait_buffers* G) {
  const int N = P->num_envs, NB = P->num_bodies, nfeet = P->num_feet;
  const float dt = P->dt;
#pragma omp parallel for schedule(static)
  for (int e = 0; e < N; ++e) {
    if (!still_recording(G->status, *B, e)) continue;
    float* body = G->body + (size_t)e * LGX_GAIT_BODY_COLS;
    const bool first = body[0] == 0.f;
    int bits = 0;
    for (int f = 0; f < nfeet; ++f) {
      const size_t row = (size_t)e * NB + P->feet_idx[f];
      const float* F = B->contact_forces + row * 3;
      bits |= gait_contact(F) ? (1 << f) : 0;
      gait_foot_sample(G->foot + ((size_t)e * LGX_MAX_FEET + f) * LGX_GAIT_FOOT_COLS, first, F,
                       B->rigid_body_states + row * 13, dt);
    }
    for (int col = 0; col < LGX_GAIT_BODY_COLS; ++col) body[col] = gait_body_col(col, body[col], bits, nfeet);
  }
}

// lgx_gait_reduce: the envs in order; returns the number of envs outside the cell grid (cells are
// written only when it is 0, overflow always is)
int gait_reduce(const lgx_task_params* P, const lgx_buffers* B, const lgx_gait_buffers* G) {
  const int N = P->num_envs, rows = G->cell_rows, cols = G->cell_cols;
  if (int bad = reduce_begin(B, G->cell_ids, N, rows, cols, G->overflow, {{G->cells, LGX_GAIT_CELL_COLS}})) return bad;
  for (int e = 0; e < N; ++e) {  // env order: deterministic
    const float* body = G->body + (size_t)e * LGX_GAIT_BODY_COLS;
    if (G->status[e] == 0 || !(body[0] > 0.f)) continue;
    const int id = cell_of_env(B->terrain_levels, B->terrain_types, G->cell_ids, e, rows, cols);
    double* cl = G->cells + (size_t)id * LGX_GAIT_CELL_COLS;
    cl[0] += 1.0;
    for (int k = 0; k < LGX_GAIT_BODY_COLS; ++k) cl[1 + k] += (double)body[k];
    for (int f = 0; f < LGX_MAX_FEET; ++f) {
      const float* r = G->foot + ((size_t)e * LGX_MAX_FEET + f) * LGX_GAIT_FOOT_COLS;
      double* cf = cl + 1 + LGX_GAIT_BODY_COLS + (LGX_GAIT_FOOT_COLS - 4) * f;
      for (int k = 4; k < LGX_GAIT_FOOT_COLS; ++k) cf[k - 4] += (double)r[k];
    }
  }
  return 0;
}

void joint_begin(const lgx_task_params* P, const lgx_joint_buffers* J) {
  zero_records(J->joint, LGX_JOINT_COLS * LGX_MAX_DOF, J->body, LGX_JOINT_BODY_COLS, J->status, J->overflow,
               (size_t)P->num_envs);
}

// The kernel's 16-lane group as one value: joint_power_sum's butterfly on all 16 slots at once.
struct Slots16 { float v[16]; };
static inline Slots16 operator+(const Slots16& a, const Slots16& b) {
  Slots16 r;
  for (int i = 0; i < 16; ++i) r.v[i] = a.v[i] + b.v[i];
  return r;
}

// lgx_joint_record (include/lgx.h): the kernel's arithmetic (lgx_env.hip joint_record_kernel), the
// joints in order
void joint_record(const lgx_task_params* P, const lgx_buffers* B, const lgx_joint_buffers* J) {
  const int N = P->num_envs, D = P->num_dof, A = P->num_actions;
#pragma omp parallel for schedule(static)
  for (int e = 0; e < N; ++e) {
    if (!still_recording(J->status, *B, e)) continue;
    float* body = J->body + (size_t)e * LGX_JOINT_BODY_COLS;
    const bool first = body[0] == 0.f;
    Slots16 s = {};
    bool any_sat = false, any_out = false;
    for (int j = 0; j < D; ++j) {
      const size_t k = (size_t)e * D + j;
      bool sat, out;
      s.v[j] = joint_sample(J->joint + ((size_t)e * LGX_MAX_DOF + j) * LGX_JOINT_COLS, first, B->torques[k],
                            B->dof_state[2 * k], B->dof_state[2 * k + 1], j < A ? B->actions[(size_t)e * A + j] : 0.f,
                            P->torque_limits[j], P->dof_vel_limits[j], P->dof_pos_limits[j][0], P->dof_pos_limits[j][1],
                            P->clip_actions, P->dt, sat, out);
      any_sat |= sat;
      any_out |= out;
    }
    const Slots16 total = joint_power_sum(s, [](const Slots16& x, int o) {
      Slots16 r;
      for (int i = 0; i < 16; ++i) r.v[i] = x.v[i ^ o];
      return r;
    });
    joint_body_sample(body, total.v[0], any_sat, any_out);
  }
}

// lgx_joint_reduce: the envs in order; returns the number of envs outside the cell grid (cells are
// written only when it is 0, overflow always is)
int joint_reduce(const lgx_task_params* P, const lgx_buffers* B, const lgx_joint_buffers* J) {
  const int N = P->num_envs, rows = J->cell_rows, cols = J->cell_cols;
  if (int bad = reduce_begin(B, J->cell_ids, N, rows, cols, J->overflow, {{J->cells, LGX_JOINT_CELL_COLS}})) return bad;
  constexpr int NS = LGX_JOINT_COLS - 1, PER = NS + 5;
  for (int e = 0; e < N; ++e) {  // env order: deterministic
    const float* body = J->body + (size_t)e * LGX_JOINT_BODY_COLS;
    if (J->status[e] == 0 || !(body[0] > 0.f)) continue;
    const int id = cell_of_env(B->terrain_levels, B->terrain_types, J->cell_ids, e, rows, cols);
    double* cl = J->cells + (size_t)id * LGX_JOINT_CELL_COLS;
    const bool init = cl[0] == 0.0;  // the cell's first env sets the maxima and minima
    const auto hi = [init](double& m, float v) { m = init ? (double)v : std::max(m, (double)v); };
    cl[0] += 1.0;
    for (int k = 0; k < LGX_JOINT_BODY_COLS; ++k) cl[1 + k] += (double)body[k];
    hi(cl[1 + LGX_JOINT_BODY_COLS], body[1]);
    for (int j = 0; j < LGX_MAX_DOF; ++j) {
      const float* r = J->joint + ((size_t)e * LGX_MAX_DOF + j) * LGX_JOINT_COLS;
      double* cj = cl + 2 + LGX_JOINT_BODY_COLS + PER * j;
      for (int k = 0; k < NS; ++k) cj[k] += (double)r[1 + k];
      hi(cj[NS], r[3]);
      hi(cj[NS + 1], r[6]);
      hi(cj[NS + 2], r[7]);
      cj[NS + 3] = init ? (double)r[10] : std::min(cj[NS + 3], (double)r[10]);
      hi(cj[NS + 4], r[11]);
    }
  }
  return 0;
}

void contact_begin(const lgx_task_params* P, const lgx_contact_buffers* C) {
  const size_t N = (size_t)P->num_envs;
  std::fill(C->body, C->body + N * LGX_MAX_BODIES * LGX_CONTACT_COLS, 0.f);
  for (size_t e = 0; e < N; ++e) {
    float* v = C->env + e * LGX_CONTACT_ENV_COLS;
    v[0] = v[1] = v[2] = v[3] = v[5] = v[7] = 0.f;
    v[4] = v[6] = -1.0f;  // the terminal columns' "none"
  }
  std::fill(C->status, C->status + N, (uint8_t)0);
  *C->overflow = 0;
}

// lgx_contact_record (include/lgx.h): the kernel's arithmetic (lgx_env.hip contact_record_kernel),
// the bodies in order
void contact_record(const lgx_task_params* P, const lgx_buffers* B, const lgx_contact_buffers* C) {
  const int N = P->num_envs, NB = P->num_bodies;
  const int16_t* hs = P->mesh_type == LGX_MESH_PLANE ? nullptr : B->height_samples;
#pragma omp parallel for schedule(static)
  for (int e = 0; e < N; ++e) {
    if (C->status[e] != 0) continue;
    float* v = C->env + (size_t)e * LGX_CONTACT_ENV_COLS;
    const bool rs = B->reset[e] != 0, first = v[0] == 0.f;
    contact_part p = contact_none();
    for (int b = 0; b < NB; ++b) {
      const size_t row = (size_t)e * NB + b;
      const float* F = B->contact_forces + row * 3;
      const float fn = rs ? nrm3(F[0], F[1], F[2])
                          : contact_body_sample(C->body + ((size_t)e * LGX_MAX_BODIES + b) * LGX_CONTACT_COLS, first, F,
                                                B->rigid_body_states + row * 13, P, hs, C->edge_tol);
      contact_merge(p, contact_body_part(P, b, fn));
    }
    if (rs) {
      const int ns = episode_end_status(*B, e);
      C->status[e] = (uint8_t)ns;
      if (ns == 2) contact_env_terminal(v + 4, p);
    } else {
      contact_env_sample(v, p);
    }
  }
}

// lgx_contact_reduce; returns the number of envs outside the cell grid (cells are written only when
// it is 0, overflow always is). The sums are formed by cell_reduce's tree (lgx_env.hip), so that both
// backends give the same bits from the same records: "thread" t = e % 256 adds the cell's envs t,
// t + 256, ... in increasing order into its own fp64 partials, the 64 partials of each "wave" are
// folded by the shuffle-down steps 32, 16, ..., 1, and the four wave results are added in wave order.
// The maxima and minima do not depend on the order.
static double contact_tree(const double* part, int k) {
  double w[4];
  for (int wv = 0; wv < 4; ++wv) {
    double s[64];
    for (int l = 0; l < 64; ++l) s[l] = part[(size_t)(64 * wv + l) * LGX_CONTACT_CELL_COLS + k];
    for (int o = 32; o > 0; o >>= 1)
      for (int l = 0; l < o; ++l) s[l] += s[l + o];
    w[wv] = s[0];
  }
  return ((w[0] + w[1]) + w[2]) + w[3];
}

int contact_reduce(const lgx_task_params* P, const lgx_buffers* B, const lgx_contact_buffers* C) {
  const int N = P->num_envs, rows = C->cell_rows, cols = C->cell_cols;
  if (int bad = reduce_begin(B, C->cell_ids, N, rows, cols, C->overflow, {{C->cells, LGX_CONTACT_CELL_COLS}})) return bad;
  constexpr int PER = 13, NCOL = LGX_CONTACT_CELL_COLS;
  static const int kSum[8] = {1, 2, 3, 5, 6, 8, 9, 11};
  // the finished envs by cell, in env order (a counting sort)
  std::vector<int> cell(N, -1), start((size_t)rows * cols + 1, 0), order;
  for (int e = 0; e < N; ++e) {
    if (C->status[e] == 0) continue;
    cell[e] = cell_of_env(B->terrain_levels, B->terrain_types, C->cell_ids, e, rows, cols);
    ++start[cell[e] + 1];
  }
  for (size_t i = 1; i < start.size(); ++i) start[i] += start[i - 1];
  order.resize(start.back());
  {
    std::vector<int> at(start.begin(), start.end() - 1);
    for (int e = 0; e < N; ++e)
      if (cell[e] >= 0) order[at[cell[e]]++] = e;
  }
  std::vector<double> part((size_t)256 * NCOL);
  for (int id = 0; id < rows * cols; ++id) {
    if (start[id] == start[id + 1]) continue;  // (an empty cell stays all zero)
    double* cl = C->cells + (size_t)id * NCOL;
    std::fill(part.begin(), part.end(), 0.0);
    bool init = true, init7 = true;  // the cell's first env / first env with samples sets the extremes
    for (int i = start[id]; i < start[id + 1]; ++i) {
      const int e = order[i], st = C->status[e];
      const float* v = C->env + (size_t)e * LGX_CONTACT_ENV_COLS;
      double* p = part.data() + (size_t)(e & 255) * NCOL;
      const bool fell = st == 2, has = v[0] > 0.f;
      const auto hi = [init](double& m, float x) { m = init ? (double)x : std::max(m, (double)x); };
      p[0] += 1.0;
      for (int k = 0; k < 3; ++k) p[1 + k] += (double)v[k];
      hi(cl[4], v[3]);
      p[5] += fell ? 1.0 : 0.0;
      p[6] += fell && v[4] < 0.f ? 1.0 : 0.0;
      p[7] += fell ? (double)v[7] : 0.0;
      for (int b = 0; b < LGX_MAX_BODIES; ++b) {
        const float* r = C->body + ((size_t)e * LGX_MAX_BODIES + b) * LGX_CONTACT_COLS;
        double *pb = p + 8 + PER * b, *cb = cl + 8 + PER * b;
        for (int k = 0; k < 8; ++k) pb[k] += (double)r[kSum[k]];
        hi(cb[8], r[4]);
        hi(cb[9], r[10]);
        if (has) cb[10] = init7 ? (double)r[7] : std::min(cb[10], (double)r[7]);
        pb[11] += fell && v[4] == (float)b ? 1.0 : 0.0;
        pb[12] += fell && v[6] == (float)b ? 1.0 : 0.0;
      }
      init = false;
      if (has) init7 = false;
    }
    for (int k = 0; k < NCOL; ++k) {
      const int kb = k < 8 ? -1 : (k - 8) % PER;
      if (k == 4 || (kb >= 8 && kb <= 10)) continue;  // the extremes, set above
      cl[k] = contact_tree(part.data(), k);
    }
  }
  return 0;
}

int threads() { return omp_get_max_threads(); }

}  // namespace lgxh
