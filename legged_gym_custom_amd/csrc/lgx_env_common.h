// lgx_env_common.h — the env step's scalar code, stated once for both backends of
// include/lgx.h: the gfx950 kernels (lgx_env.hip) and the host backend (lgx_env_host.cpp).
// Plain C++17 with no lane index in it: the 3-vector math, the Philox counter RNG, the step's
// constants and uniform slots, the terrain triangle geometry, the post-physics helpers, command
// resampling, the reward terms, the scalar head of reset_idx and the command curriculum.
// Not here, on purpose: the physics and every lane-parallel phase (the kernel spreads an env
// over a wave's lanes, the host loops), and the oracle under oracle/, which stays an
// independent statement and never includes this file.
// Both backends build with -ffp-contract=off, so one body gives each backend the bits its own copy
// gave; the one exception is marked below ("inside the physics").
#pragma once
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/lgx.h"

#ifdef __HIPCC__
#define LGX_HD __host__ __device__ __forceinline__
#define LGX_UNROLL _Pragma("unroll")
#else
#define LGX_HD static inline
#define LGX_UNROLL
#endif

// ---------------------------------------------------------------- Philox4x32-10
// Same definition as oracle/philox.py and oracle/lgx_oracle.c (counter layout:
// c0 = global env id, c1/c3 = step lo/hi, c2 = block | stream << 16; key = seed).
LGX_HD uint32_t mulhi32(uint32_t a, uint32_t b) { return (uint32_t)(((uint64_t)a * b) >> 32); }
LGX_HD void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                          uint32_t out[4]) {
  LGX_UNROLL
  for (int r = 0; r < 10; ++r) {
    uint32_t hi0 = mulhi32(0xD2511F53u, c0), lo0 = 0xD2511F53u * c0;
    uint32_t hi1 = mulhi32(0xCD9E8D57u, c2), lo1 = 0xCD9E8D57u * c2;
    uint32_t n0 = hi1 ^ c1 ^ k0;
    uint32_t n2 = hi0 ^ c3 ^ k1;
    c0 = n0; c1 = lo1; c2 = n2; c3 = lo0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}
LGX_HD float u01(uint32_t x) { return (float)(x >> 8) * (1.0f / 16777216.0f); }

// ---------------------------------------------------------------- fp32 vector math
struct f3 {
  float x, y, z;
};
LGX_HD f3 mk(float x, float y, float z) { return f3{x, y, z}; }
LGX_HD f3 ld3(const float* p) { return f3{p[0], p[1], p[2]}; }
LGX_HD void st3(float* p, f3 v) { p[0] = v.x; p[1] = v.y; p[2] = v.z; }
LGX_HD f3 operator+(f3 a, f3 b) { return f3{a.x + b.x, a.y + b.y, a.z + b.z}; }
LGX_HD f3 operator-(f3 a, f3 b) { return f3{a.x - b.x, a.y - b.y, a.z - b.z}; }
LGX_HD f3 operator*(f3 a, float s) { return f3{a.x * s, a.y * s, a.z * s}; }
LGX_HD float dot(f3 a, f3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
LGX_HD f3 cross(f3 a, f3 b) { return f3{a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
// row-major 3x3
LGX_HD f3 mv(const float* R, f3 v) {
  return f3{R[0] * v.x + R[1] * v.y + R[2] * v.z, R[3] * v.x + R[4] * v.y + R[5] * v.z,
            R[6] * v.x + R[7] * v.y + R[8] * v.z};
}
LGX_HD void mm(const float* A, const float* B, float* O) {
  float T[9];
  LGX_UNROLL
  for (int i = 0; i < 3; ++i)
    LGX_UNROLL
    for (int j = 0; j < 3; ++j) T[i * 3 + j] = A[i * 3] * B[j] + A[i * 3 + 1] * B[3 + j] + A[i * 3 + 2] * B[6 + j];
  LGX_UNROLL
  for (int i = 0; i < 9; ++i) O[i] = T[i];
}
// symmetric inertia (xx yy zz xy xz yz) times vector
LGX_HD f3 symv(const float* I, f3 v) {
  return f3{I[0] * v.x + I[3] * v.y + I[4] * v.z, I[3] * v.x + I[1] * v.y + I[5] * v.z,
            I[4] * v.x + I[5] * v.y + I[2] * v.z};
}
LGX_HD void quat_to_R(const float* q, float* R) {
  float x = q[0], y = q[1], z = q[2], w = q[3];
  R[0] = 1 - 2 * (y * y + z * z); R[1] = 2 * (x * y - z * w); R[2] = 2 * (x * z + y * w);
  R[3] = 2 * (x * y + z * w); R[4] = 1 - 2 * (x * x + z * z); R[5] = 2 * (y * z - x * w);
  R[6] = 2 * (x * z - y * w); R[7] = 2 * (y * z + x * w); R[8] = 1 - 2 * (x * x + y * y);
}

// ---------------------------------------------------------------- inside the physics
// The one difference between the backends in this header: the kernel's physics contracts
// a * b + c into fma (lgx_env.hip, "physics helpers"), the host backend never does, so the
// bodies of this section are contracted under hipcc only. The backends' physics is
// pinned to each other at 2e-3 (tests/test_host_parity.py), not bit for bit.
#ifdef __HIPCC__
#pragma clang fp contract(fast)
#endif

// symmetric 3x3 (xx yy zz xy xz yz) inverse
LGX_HD void sym3_inv(const float* D, float* O) {
  float a = D[0], b = D[1], c = D[2], d = D[3], e = D[4], f = D[5];
  float A = b * c - f * f, Bm = -(d * c - e * f), Cm = d * f - b * e;
  float det = a * A + d * Bm + e * Cm;
  float inv = 1.0f / det;
  O[0] = A * inv;
  O[1] = (a * c - e * e) * inv;
  O[2] = (a * b - d * d) * inv;
  O[3] = Bm * inv;
  O[4] = Cm * inv;
  O[5] = -(a * f - d * e) * inv;
}
LGX_HD float sym3(const float* S, int i, int j) {
  if (i == j) return S[i];
  int k = i + j;  // (0,1)->3 (0,2)->4 (1,2)->5
  return S[k == 1 ? 3 : (k == 2 ? 4 : 5)];
}
// packed symmetric 6x6 index (lower, row-major)
LGX_HD int pk(int i, int j) { return i >= j ? i * (i + 1) / 2 + j : j * (j + 1) / 2 + i; }

// The reference's trimesh (terrain_utils.py:382-465) is never materialised: vertex (i, j) sits
// at ((i + dx) hs, (j + dy) hs, h vs) - border, where h (int16) and the slope-threshold shift
// (dx, dy in {-1, 0, 1}) are packed in one 32-bit word per vertex (lgx_buffers.terrain_mesh).
// Here relative to the query's cell (ci, cj).
LGX_HD f3 mesh_vertex(const uint32_t* mesh, int cols, int i, int j, int ci, int cj, float hs, float vs) {
  const uint32_t w = mesh[(size_t)i * cols + j];
  const float h = (float)(int16_t)(w & 0xffffu);
  const int dx = (int)((w >> 16) & 3u) - 1, dy = (int)((w >> 18) & 3u) - 1;
  return mk((float)(i - ci + dx) * hs, (float)(j - cj + dy) * hs, h * vs);
}

// closest point of triangle abc to p (Ericson, Real-Time Collision Detection 5.1.5),
// with guards for the zero-area triangles a wall shift can produce
LGX_HD f3 closest_on_triangle(f3 p, f3 a, f3 b, f3 c) {
  const f3 ab = b - a, ac = c - a, ap = p - a;
  const float d1 = dot(ab, ap), d2 = dot(ac, ap);
  if (d1 <= 0.f && d2 <= 0.f) return a;
  const f3 bp = p - b;
  const float d3 = dot(ab, bp), d4 = dot(ac, bp);
  if (d3 >= 0.f && d4 <= d3) return b;
  const float vc = d1 * d4 - d3 * d2;
  if (vc <= 0.f && d1 >= 0.f && d3 <= 0.f) return a + ab * (d1 / fmaxf(d1 - d3, 1e-30f));
  const f3 cp = p - c;
  const float d5 = dot(ab, cp), d6 = dot(ac, cp);
  if (d6 >= 0.f && d5 <= d6) return c;
  const float vb = d5 * d2 - d1 * d6;
  if (vb <= 0.f && d2 >= 0.f && d6 <= 0.f) return a + ac * (d2 / fmaxf(d2 - d6, 1e-30f));
  const float va = d3 * d6 - d5 * d4;
  if (va <= 0.f && d4 - d3 >= 0.f && d5 - d6 >= 0.f)
    return b + (c - b) * ((d4 - d3) / fmaxf((d4 - d3) + (d5 - d6), 1e-30f));
  const float inv = 1.0f / fmaxf(va + vb + vc, 1e-30f);
  return a + ab * (vb * inv) + ac * (vc * inv);
}

// surface height of triangle abc above (p.x, p.y) if its xy projection contains it
LGX_HD bool height_in_triangle(f3 p, f3 a, f3 b, f3 c, float& z) {
  const float e1x = b.x - a.x, e1y = b.y - a.y, e2x = c.x - a.x, e2y = c.y - a.y;
  const float det = e1x * e2y - e1y * e2x;
  if (fabsf(det) < 1e-10f) return false;  // vertical wall: no projection
  const float px = p.x - a.x, py = p.y - a.y;
  const float u = (px * e2y - py * e2x) / det, v = (e1x * py - e1y * px) / det;
  const float eps = -1e-6f;
  if (u < eps || v < eps || u + v > 1.0f - eps) return false;
  z = a.z + u * (b.z - a.z) + v * (c.z - a.z);
  return true;
}

#ifdef __HIPCC__
#pragma clang fp contract(off)
#endif

// ---------------------------------------------------------------- the step's constants, post-physics
// (isaacgym torch_utils / legged_gym math in fp32, no contraction: the reference evaluates
// these as separate eager torch ops)
namespace lgx {

constexpr int NL = 13;  // dynamic links: base + 4 chains x 3 (checked by lgx_create)
constexpr int NJ = 12;
constexpr int NU = 18;
constexpr int MAXC = LGX_MAX_CONTACTS;
constexpr int MAXR = NJ + 3 * MAXC;
// Philox blocks per env per step: 9 fixed blocks (commands, push/terrain, dof, root, reset
// commands) + one per 4 observation-noise draws (oracle/philox.py num_blocks): Go2 22,
// ANYmal (235 proprio) 68
constexpr int NBLK_MAX = 9 + (LGX_MAX_PROPRIO + 3) / 4;
constexpr int NSLOT = NBLK_MAX * 4;
LGX_HD int rng_blocks(const lgx_task_params* Pm) { return 9 + (Pm->num_proprio + 3) / 4; }
constexpr int MAXHIST = 1216;

enum Slot { S_CMD = 0, S_PUSH = 4, S_TERR = 6, S_DOF = 8, S_ROOT_XY = 20, S_ROOT_VEL = 24, S_RCMD = 32, S_NOISE = 36 };

struct Scratch {  // per-env post-physics scalars (go2.py:357-367, 279-328)
  float blv[3], bav[3], pg[3];
  float roll, pitch, yaw;
  float ph[4];  // fl fr bl br
  int contact[4];
  float feet_z[4];
  float jump;
};

// sums over joints / height points shared by the reward terms (each backend's joint_sums)
enum JSum { J_ACTION_RATE, J_DELTA_TORQUES, J_DOF_ACC, J_DOF_ERROR, J_DOF_POS_LIMITS, J_DOF_VEL, J_DOF_VEL_LIMITS,
            J_STAND_ABS, J_TORQUE_LIMITS, J_TORQUES, J_HIP_POS, J_THIGH_POS, J_CALF_POS, J_HEIGHT, J_N };

LGX_HD void quat_rotate_inverse(const float* q, const float* v, float* out) {
  float w = q[3];
  float sc = 2.0f * (w * w) - 1.0f;
  float cx = q[1] * v[2] - q[2] * v[1];
  float cy = q[2] * v[0] - q[0] * v[2];
  float cz = q[0] * v[1] - q[1] * v[0];
  float d = q[0] * v[0] + q[1] * v[1] + q[2] * v[2];
  out[0] = v[0] * sc - cx * w * 2.0f + q[0] * d * 2.0f;
  out[1] = v[1] * sc - cy * w * 2.0f + q[1] * d * 2.0f;
  out[2] = v[2] * sc - cz * w * 2.0f + q[2] * d * 2.0f;
}
LGX_HD void quat_apply(const float* q, const float* b, float* out) {
  float t0 = (q[1] * b[2] - q[2] * b[1]) * 2.0f;
  float t1 = (q[2] * b[0] - q[0] * b[2]) * 2.0f;
  float t2 = (q[0] * b[1] - q[1] * b[0]) * 2.0f;
  out[0] = b[0] + q[3] * t0 + (q[1] * t2 - q[2] * t1);
  out[1] = b[1] + q[3] * t1 + (q[2] * t0 - q[0] * t2);
  out[2] = b[2] + q[3] * t2 + (q[0] * t1 - q[1] * t0);
}
LGX_HD float trem(float a, float b) {  // torch.remainder
  float m = fmodf(a, b);
  if (m != 0.0f && ((m < 0.0f) != (b < 0.0f))) m += b;
  return m;
}
LGX_HD float wrap_to_pi(float a) {
  const float two_pi = 6.283185307179586f, pi = 3.141592653589793f;
  float m = trem(a, two_pi);
  m -= two_pi * (float)(m > pi);
  return m;
}
LGX_HD float clipf(float x, float lo, float hi) { return x < lo ? lo : (x > hi ? hi : x); }
LGX_HD float sq(float x) { return x * x; }
LGX_HD float nrm3(float a, float b, float c) { return sqrtf(a * a + b * b + c * c); }
LGX_HD float nrm2(float a, float b) { return sqrtf(a * a + b * b); }
LGX_HD float rand_range(float lo, float hi, float u) {
  float span = (float)((double)hi - (double)lo);
  return span * u + lo;
}
// torch_rand_float(lo, hi) with the reference's Python-float (double) bounds: (hi - lo) and lo
// enter the fp32 tensor ops as fp32 scalars
LGX_HD float rand_range_d(double lo, double hi, float u) { return (float)(hi - lo) * u + (float)lo; }

// Actuation latency (lgx_buffers.action_delay, include/lgx.h). d: an env's latency in physics
// substeps, clamped by action_delay_clamp into [0, H * decimation]. action_age: how many control
// steps old the action is that the actuator sees in substep `sub` of a step,
// ceil(max(d - sub, 0) / decimation) in 0..H: 0 = this step's action, i >= 1 = action_history
// row i - 1.
LGX_HD int action_delay_clamp(int d, int H, int decimation) {
  const int hi = H * decimation;
  return d < 0 ? 0 : (d > hi ? hi : d);
}
LGX_HD int action_age(int d, int sub, int decimation) {
  // ceil(x / n) for x <= LGX_MAX_ACTION_HISTORY * n counts the multiples i * n below x: no integer
  // division (on the GPU that is a float reciprocal sequence in vector registers)
  const int left = d - sub;
  int age = 0;
  LGX_UNROLL
  for (int i = 0; i < LGX_MAX_ACTION_HISTORY; ++i) age += (int)(left > i * decimation);
  return age;
}
// The end of a step for element j of env e's history ([H, A] at h): rows shift down by one (zeroed
// instead when the env reset in this step) and row 0 takes `last`, the value last_actions gets.
LGX_HD void action_history_push(float* h, int H, int A, int j, float last, bool reset) {
  for (int i = H - 1; i >= 1; --i) h[i * A + j] = reset ? 0.f : h[(i - 1) * A + j];
  h[j] = last;
}

// Scheduled push (lgx_buffers.push_step / push_dvel, include/lgx.h ABI 9): the impulse dv =
// (forward, left, yaw rate) in the robot's heading frame added to the staged root state's world
// velocity. Called by both backends right after the reference's push, for an env whose incremented
// episode length equals its push_step.
LGX_HD void scheduled_push(float* root, const float* dv) {
  const float fwd[3] = {1.f, 0.f, 0.f};
  float f[3];
  quat_apply(root + 3, fwd, f);
  const float n = nrm2(f[0], f[1]);
  const bool ok = n > 1e-6f;
  const float hx = ok ? f[0] / n : 1.0f, hy = ok ? f[1] / n : 0.0f;
  root[7] = root[7] + (dv[0] * hx - dv[1] * hy);
  root[8] = root[8] + (dv[0] * hy + dv[1] * hx);
  root[12] = root[12] + dv[2];
}

// External force (lgx_buffers.force_window / force_vec, include/lgx.h ABI 16). The window: is the
// force of an env with the row (start, steps, period) on in the step that writes episode length
// ep? start + steps is never formed (steps = INT32_MAX: to the end of the episode).
LGX_HD bool force_window_on(int32_t start, int32_t steps, int32_t period, long long ep) {
  if (start < 1 || steps < 1) return false;
  const long long k = ep - (long long)start;
  if (k < 0) return false;
  return (period >= 1 ? k % (long long)period : k) < (long long)steps;
}
// The frame: fv = (forward, left, up) in the heading frame of the root quaternion q (x, y, z, w)
// to the world vector out, with the heading rule of scheduled_push; up goes along world z.
LGX_HD void force_to_world(const float* q, const float* fv, float* out) {
  const float fwd[3] = {1.f, 0.f, 0.f};
  float f[3];
  quat_apply(q, fwd, f);
  const float n = nrm2(f[0], f[1]);
  const bool ok = n > 1e-6f;
  const float hx = ok ? f[0] / n : 1.0f, hy = ok ? f[1] / n : 0.0f;
  out[0] = fv[0] * hx - fv[1] * hy;
  out[1] = fv[0] * hy + fv[1] * hx;
  out[2] = fv[2];
}

// Push recovery (lgx_eval_buffers.push_rec, include/lgx.h ABI 9): one post-push sample of an env,
// k > 0 steps after its push. The new value of record column col (0..3) from its old value x; pg:
// projected gravity, c / v: commands and base_lin_vel. (The kernel gives one column to each of an
// env's four lanes, the host backend loops over them.)
LGX_HD float push_record_col(int col, float x, const float* pg, const float* c, const float* v, long long k,
                             float settle_tol) {
  if (col == 0) return x + 1.0f;
  if (col == 1) return fmaxf(x, atan2f(nrm2(pg[0], pg[1]), -pg[2]));
  const float err = sqrtf((c[0] - v[0]) * (c[0] - v[0]) + (c[1] - v[1]) * (c[1] - v[1]));
  if (col == 2) return fmaxf(x, err);
  return err > settle_tol ? (float)k : x;
}

// Command schedule (lgx_buffers.cmd_step / cmd_val, include/lgx.h ABI 10): the active segment of
// an env at episode length ep is the largest k with 0 <= steps_row[k] <= ep (start steps are
// non-decreasing over the used entries; an entry < 0 is unused). If there is one, cmd takes its
// four values exactly; if not, cmd is left alone. Called by both backends after every command
// resample (post-physics: also after the heading rule), for an env whose buffers are bound.
LGX_HD void scheduled_command(float* cmd, const int32_t* steps_row, const float* vals_row, long long ep) {
  int k = -1;
  for (int i = 0; i < LGX_CMD_SEGMENTS; ++i) {
    const int st = steps_row[i];
    if (st >= 0 && (long long)st <= ep) k = i;
  }
  if (k < 0) return;
  for (int i = 0; i < 4; ++i) cmd[i] = vals_row[k * 4 + i];
}

// Step response (lgx_eval_buffers.cmd_rec, include/lgx.h ABI 10): one sample of an env, k >= 0
// steps after its command switch. The new value of record column col (0..7) from its old value x;
// pg: projected gravity, c: commands, v / w: base_lin_vel / base_ang_vel. (The kernel gives columns
// 2q and 2q+1 to lane q of an env's four lanes, the host backend loops over them.)
LGX_HD float command_record_col(int col, float x, const float* pg, const float* c, const float* v, const float* w,
                                long long k, float settle_tol, float yaw_tol, int steady_after) {
  if (col == 0) return x + 1.0f;
  if (col == 1) {
    const float err = sqrtf((c[0] - v[0]) * (c[0] - v[0]) + (c[1] - v[1]) * (c[1] - v[1]));
    return err > settle_tol ? (float)(k + 1) : x;
  }
  if (col == 2) return fabsf(c[2] - w[2]) > yaw_tol ? (float)(k + 1) : x;
  if (col == 3) return fmaxf(x, atan2f(nrm2(pg[0], pg[1]), -pg[2]));
  if (k < (long long)steady_after) return x;
  if (col == 4) return x + 1.0f;
  if (col == 5) return x + v[0];
  if (col == 6) return x + v[1];
  return x + w[2];
}

// Flight recorder (lgx_trace_buffers, include/lgx.h ABI 11): column col < 74 of env e's row, from the
// buffers as the step left them: the copied columns (0-68, 73) and the foot force norms (69-72).
// (The kernel gives column l + 16 p to lane l of an env's sixteen lanes in pass p, the host backend
// loops over the columns. Columns 74 and 75 come from trace_peak_merge below.)
LGX_HD float trace_col(int col, const lgx_task_params* Pm, const lgx_buffers& B, int e) {
  const int D = Pm->num_dof;
  const size_t se = (size_t)e;
  if (col == 0) return (float)B.episode_length[se];
  if (col < 8) return B.root_states[se * 13 + (col - 1)];
  if (col < 11) return B.base_lin_vel[se * 3 + (col - 8)];
  if (col < 14) return B.base_ang_vel[se * 3 + (col - 11)];
  if (col < 17) return B.projected_gravity[se * 3 + (col - 14)];
  if (col < 21) return B.commands[se * 4 + (col - 17)];
  if (col < 69) {
    const int k = (col - 21) / LGX_MAX_DOF, j = (col - 21) % LGX_MAX_DOF;
    if (j >= D) return 0.f;
    if (k < 2) return B.dof_state[(se * D + j) * 2 + k];
    return k == 2 ? B.torques[se * D + j] : B.actions[se * Pm->num_actions + j];
  }
  if (col < 73) {
    const int f = col - 69;
    if (f >= Pm->num_feet) return 0.f;
    const float* c = B.contact_forces + (se * Pm->num_bodies + Pm->feet_idx[f]) * 3;
    return nrm3(c[0], c[1], c[2]);
  }
  return B.rew[se];
}
// Whether reported body b is one of the feet (the peak of columns 74 / 75 runs over the others).
LGX_HD bool trace_is_foot(const lgx_task_params* Pm, int b) {
  bool foot = false;
  for (int f = 0; f < Pm->num_feet; ++f) foot = foot || Pm->feet_idx[f] == b;
  return foot;
}
// Columns 74 / 75: fold the candidate (norm n of body b) into the running peak (pn, pb), which
// starts at (0, -1). The larger norm wins, the lower body index wins a tie, a zero norm never wins:
// associative and commutative, so the kernel's lane tree and the host's loop agree.
LGX_HD void trace_peak_merge(float& pn, int& pb, float n, int b) {
  if (n > pn || (n == pn && n > 0.f && b < pb)) {
    pn = n;
    pb = b;
  }
}

// The episode-end rule of the three records (eval, trace and gait status): how the episode of env e
// ended in the step just run, which reset it: 3 blew up (when blew_up is bound), 1 timed out, 2 fell.
LGX_HD int episode_end_status(const uint8_t* blew_up, const uint8_t* time_out, int e) {
  return (blew_up && blew_up[e]) ? 3 : (time_out[e] ? 1 : 2);
}
LGX_HD int episode_end_status(const lgx_buffers& B, int e) { return episode_end_status(B.blew_up, B.time_out, e); }
// The env-to-cell rule of lgx_eval_reduce / lgx_gait_reduce: cell_ids[e] when set, else level * cols
// + type (0 for an unbound one); -1 when it lies outside the rows x cols grid (never used as an index).
LGX_HD int cell_of_env(const int64_t* levels, const int64_t* types, const int32_t* cell_ids, int e, int rows,
                       int cols) {
  if (cell_ids) {
    const int id = cell_ids[e];
    return (id < 0 || id >= rows * cols) ? -1 : id;
  }
  const int64_t lv = levels ? levels[e] : 0, ty = types ? types[e] : 0;
  return (lv < 0 || lv >= rows || ty < 0 || ty >= cols) ? -1 : (int)(lv * cols + ty);
}

// Gait record (lgx_gait_buffers, include/lgx.h ABI 12). The contact rule of a foot from its net
// contact force F: the step's own (curc, unfiltered).
LGX_HD bool gait_contact(const float* F) { return F[2] > 1.0f; }
// One sample of one foot: the 16 record columns r (in registers in the kernel, in place on the
// host) from the foot's contact force F and its rigid-body row R (position 0-2, world linear
// velocity 7-9); first: the env's first sample. The order of the rule text of lgx_gait_record.
LGX_HD void gait_foot_sample(float* r, bool first, const float* F, const float* R, float dt) {
  const bool c = gait_contact(F);
  const float z = R[2], vh = nrm2(R[7], R[8]), fh = nrm2(F[0], F[1]), fn = nrm3(F[0], F[1], F[2]);
  if (first) {
    r[1] = 0.f;
  } else {
    const bool p = r[0] != 0.f;
    if (c && !p) {  // touchdown
      r[5] += 1.0f;
      r[13] = fmaxf(r[13], fn);
      if (r[1] > 0.f) {
        r[8] += 1.0f;
        r[9] += r[1];
        r[10] += r[3] - r[2];
      }
      r[1] = 1.0f;
    } else if (!c && p) {  // lift-off
      if (r[1] > 0.f) {
        r[6] += 1.0f;
        r[7] += r[1];
      }
      r[1] = 1.0f;
      r[3] = z;
    } else {
      r[1] = r[1] > 0.f ? r[1] + 1.0f : 0.f;
    }
  }
  r[0] = c ? 1.0f : 0.f;
  if (c) {
    r[4] += 1.0f;
    r[11] += vh * dt;
    r[12] += F[2];
    r[2] = z;
  } else {
    r[3] = first ? z : fmaxf(r[3], z);
    r[14] += vh * dt;
  }
  if (fh > 5.0f * fabsf(F[2])) r[15] += 1.0f;
}
// The new value of body column col (0..11) from its old value x; bits: bit f = foot f < nfeet is in
// contact. (The kernel gives columns 3q..3q+2 to lane q of an env's four lanes, the host loops.)
LGX_HD float gait_body_col(int col, float x, int bits, int nfeet) {
  if (col == 0) return x + 1.0f;
  if (col < 6) {
    const int m = (bits & 1) + ((bits >> 1) & 1) + ((bits >> 2) & 1) + ((bits >> 3) & 1);
    return m == col - 1 ? x + 1.0f : x;
  }
  const int i = col - 6;  // pairs (0,1) (0,2) (0,3) (1,2) (1,3) (2,3)
  const int a = i < 3 ? 0 : (i < 5 ? 1 : 2), b = i < 3 ? i + 1 : (i < 5 ? i - 1 : 3);
  if (b >= nfeet) return x;
  return ((bits >> a) & 1) == ((bits >> b) & 1) ? x + 1.0f : x;
}

// Joint-load record (lgx_joint_buffers, include/lgx.h ABI 13). One sample of one joint: the 16
// record columns r (in registers in the kernel, in place on the host) from the joint's torque tau,
// angle q, speed qd and action a and its limits (L torque, V speed, lo / hi angle, C action clip);
// first: the env's first sample. Returns fabsf(tau*qd), the joint's term of the total power; sat /
// out: the conditions of columns 1 and 9. The order of the rule text of lgx_joint_record.
LGX_HD float joint_sample(float* r, bool first, float tau, float q, float qd, float a, float L, float V, float lo,
                          float hi, float C, float dt, bool& sat, bool& out) {
  const float p = tau * qd, at = fabsf(tau), av = fabsf(qd), ap = fabsf(p), da = a - r[0];
  sat = at >= L;
  out = q < lo || q > hi;
  r[12] += first ? 0.f : da * da;
  r[0] = a;
  r[1] += sat ? 1.0f : 0.f;
  r[2] += tau * tau;
  r[3] = fmaxf(r[3], at);
  r[4] += fmaxf(p, 0.f) * dt;
  r[5] += fmaxf(-p, 0.f) * dt;
  r[6] = fmaxf(r[6], ap);
  r[7] = fmaxf(r[7], av);
  r[8] += av > V ? 1.0f : 0.f;
  r[9] += out ? 1.0f : 0.f;
  r[10] = first ? q : fminf(r[10], q);
  r[11] = first ? q : fmaxf(r[11], q);
  r[13] += fabsf(a) >= C ? 1.0f : 0.f;
  r[14] += p < 0.f ? 1.0f : 0.f;
  r[15] += av;
  return ap;
}
// The total power P of a sample: the sum of 16 slots by the fixed pairwise tree of the rule text,
// written as four butterfly stages. xchg(s, o) is the value of s held by the slot whose index
// differs in bit o: a xor shuffle inside the kernel's 16-lane group (T = float, a lane's slot), a
// permutation of all 16 slots on the host (T = its array of them). Every slot ends with the same
// bits (fp32 addition commutes).
template <class T, class Xchg>
LGX_HD T joint_power_sum(T s, Xchg xchg) {
  LGX_UNROLL
  for (int o = 1; o < 16; o <<= 1) s = s + xchg(s, o);
  return s;
}
// The body columns [4] after a sample: P as above, sat / out: any joint met column 1's / 9's condition.
LGX_HD void joint_body_sample(float* b, float P, bool sat, bool out) {
  b[0] += 1.0f;
  b[1] = fmaxf(b[1], P);
  b[2] += sat ? 1.0f : 0.f;
  b[3] += out ? 1.0f : 0.f;
}

// The terrain height in the cell of the point (px, py), world coordinates plus the border,
// LeggedRobot._get_heights legged_robot.py:1015-1032: truncation, every index clamped before use, the
// min of three samples, one float multiply. ix, iy: the clamped cell. hs: height_samples, not NULL.
// The step's height scan, the contact record and the scan model's second lookup (include/lgx.h,
// ABI 17) all go through this.
LGX_HD float terrain_cell_height(const lgx_task_params* Pm, const int16_t* hs, float px, float py, long& ix, long& iy) {
  ix = (long)(px / Pm->horizontal_scale);
  iy = (long)(py / Pm->horizontal_scale);
  ix = ix < 0 ? 0 : (ix > Pm->hf_rows - 2 ? Pm->hf_rows - 2 : ix);
  iy = iy < 0 ? 0 : (iy > Pm->hf_cols - 2 ? Pm->hf_cols - 2 : iy);
  const int16_t h1 = hs[ix * Pm->hf_cols + iy];
  const int16_t h2 = hs[(ix + 1) * Pm->hf_cols + iy];
  const int16_t h3 = hs[ix * Pm->hf_cols + iy + 1];
  int16_t h = h1 < h2 ? h1 : h2;
  h = h < h3 ? h : h3;
  return (float)h * Pm->vertical_scale;
}
// The yaw-only quaternion of the height scan from the root quaternion's z and w.
LGX_HD void scan_yaw_quat(float qz, float qw, float* qy) {
  float n = sqrtf(qz * qz + qw * qw);
  n = n < 1e-9f ? 1e-9f : n;
  qy[0] = 0.f; qy[1] = 0.f; qy[2] = qz / n; qy[3] = qw / n;
}
// One point of the height scan: the terrain height under the base-frame point (bx, by) of a robot
// whose world position is pos[0..1], with the yaw-only quaternion qy.
LGX_HD float scan_point_height(const lgx_task_params* Pm, const int16_t* hs, const float* qy, const float* pos,
                               float bx, float by) {
  float p[3] = {bx, by, 0.f}, w[3];
  quat_apply(qy, p, w);
  float px = (w[0] + pos[0]) + Pm->border_size, py = (w[1] + pos[1]) + Pm->border_size;
  long ix, iy;
  return terrain_cell_height(Pm, hs, px, py, ix, iy);
}

// Contact record (lgx_contact_buffers, include/lgx.h ABI 14). The terrain height under (x, y): the
// arithmetic of the step's height scan (terrain_cell_height); ix, iy: the clamped cell, for
// contact_relief. hs == nullptr (a plane): 0.
LGX_HD float contact_terrain_height(const lgx_task_params* Pm, const int16_t* hs, float x, float y, long& ix,
                                    long& iy) {
  ix = iy = 0;
  if (hs == nullptr) return 0.f;
  const float px = x + Pm->border_size, py = y + Pm->border_size;
  return terrain_cell_height(Pm, hs, px, py, ix, iy);
}
// The terrain relief around the cell (ix, iy) of contact_terrain_height: max - min of the nine
// samples around the cell moved into [1, rows - 2] x [1, cols - 2] (hf_rows, hf_cols >= 3: checked
// by the calls), the difference in int before the one float multiply.
LGX_HD float contact_relief(const lgx_task_params* Pm, const int16_t* hs, long ix, long iy) {
  if (hs == nullptr) return 0.f;
  const long cx = ix < 1 ? 1 : (ix > Pm->hf_rows - 2 ? Pm->hf_rows - 2 : ix);
  const long cy = iy < 1 ? 1 : (iy > Pm->hf_cols - 2 ? Pm->hf_cols - 2 : iy);
  int lo = 32767, hi = -32768;
  LGX_UNROLL
  for (int i = -1; i <= 1; ++i) {
    LGX_UNROLL
    for (int j = -1; j <= 1; ++j) {
      const int v = hs[(cx + i) * Pm->hf_cols + (cy + j)];
      lo = v < lo ? v : lo;
      hi = v > hi ? v : hi;
    }
  }
  return (float)(hi - lo) * Pm->vertical_scale;
}
// One sample of one body: the 12 record columns r (in registers in the kernel, in place on the
// host) from its contact force F and its position X (rigid-body row columns 0-2); first: the env's
// first sample; hs: height_samples, nullptr for a plane. Returns fn. The rule text of
// lgx_contact_record.
LGX_HD float contact_body_sample(float* r, bool first, const float* F, const float* X,
                                 const lgx_task_params* Pm, const int16_t* hs, float edge_tol) {
  const float fn = nrm3(F[0], F[1], F[2]), fh = nrm2(F[0], F[1]);
  const bool c = fn > 0.1f, onset = c && (first || r[0] == 0.f);
  long ix, iy;
  const float dz = X[2] - contact_terrain_height(Pm, hs, X[0], X[1], ix, iy);
  r[0] = c ? 1.0f : 0.f;
  r[1] += c ? 1.0f : 0.f;
  r[3] += c ? fn * Pm->dt : 0.f;
  r[4] = fmaxf(r[4], fn);
  r[5] += c && fh > 5.0f * fabsf(F[2]) ? 1.0f : 0.f;
  r[6] += dz;
  r[7] = first ? dz : fminf(r[7], dz);
  if (onset) {
    const float relief = contact_relief(Pm, hs, ix, iy);
    r[2] += 1.0f;
    r[8] += relief > edge_tol ? 1.0f : 0.f;
    r[9] += relief;
    r[10] = fmaxf(r[10], relief);
  }
  r[11] += fn > 1.0f ? 1.0f : 0.f;
  return fn;
}
// What the bodies of an env contribute to its env columns: pen / term: the entries of penalised_idx
// with c / of termination_idx with fn > 1; (tn, tb): the hardest-hit termination body over 1 N;
// (nn, nb): the hardest-hit non-foot body with fn > 0; (0, -1): none. contact_merge is associative
// and commutative (integer sums, trace_peak_merge's total order), so the kernel's xor butterfly and
// the host's loop over the bodies agree.
struct contact_part {
  int pen, term, tb, nb;
  float tn, nn;
};
LGX_HD contact_part contact_none() { return contact_part{0, 0, -1, -1, 0.f, 0.f}; }
LGX_HD contact_part contact_body_part(const lgx_task_params* Pm, int b, float fn) {
  contact_part p = contact_none();
  bool term = false;
  for (int i = 0; i < Pm->n_penalised; ++i) p.pen += (Pm->penalised_idx[i] == b && fn > 0.1f) ? 1 : 0;
  for (int i = 0; i < Pm->n_termination; ++i) term = term || Pm->termination_idx[i] == b;
  for (int i = 0; i < Pm->n_termination; ++i) p.term += (Pm->termination_idx[i] == b && fn > 1.0f) ? 1 : 0;
  if (term && fn > 1.0f) {
    p.tn = fn;
    p.tb = b;
  }
  if (!trace_is_foot(Pm, b) && fn > 0.f) {
    p.nn = fn;
    p.nb = b;
  }
  return p;
}
LGX_HD void contact_merge(contact_part& a, const contact_part& o) {
  a.pen += o.pen;
  a.term += o.term;
  trace_peak_merge(a.tn, a.tb, o.tn, o.tb);
  trace_peak_merge(a.nn, a.nb, o.nn, o.nb);
}
// Env columns 0..3 after a sample, and the terminal columns 4..7 of an env that fell.
LGX_HD void contact_env_sample(float* v, const contact_part& p) {
  v[0] += 1.0f;
  v[1] += (float)p.pen;
  v[2] += p.nn > 0.1f ? 1.0f : 0.f;  // (the largest non-foot fn is over 0.1 iff any non-foot body has c)
  v[3] = fmaxf(v[3], p.nn);
}
LGX_HD void contact_env_terminal(float* v, const contact_part& p) {
  v[0] = (float)p.tb;
  v[1] = p.tn;
  v[2] = (float)p.nb;
  v[3] = (float)p.term;
}

// Sensor model (lgx_buffers.obs_noise_scale .. sensor_count, include/lgx.h, ABI 15).
// A sensor channel of the proprio row is a measured one: Go2 angular velocity, roll, pitch and the
// joint positions / velocities; LEGGED linear and angular velocity, gravity, joint positions /
// velocities and the heights. Commands, last actions and the gait clock are not.
LGX_HD bool sensor_channel(bool go2, int i, int D, int A) {
  if (go2) return i < 5 || (i >= 8 && i < 8 + 2 * D);
  return i < 9 || (i >= 12 && i < 12 + 2 * D) || i >= 12 + 2 * D + A;
}
// The sensing latency an env has in this step: obs_delay clamped into [0, K] and to the c rows its
// episode has written so far, so a delayed read never crosses a reset.
LGX_HD int sensor_delay_clamp(int d, int K, int c) {
  d = d < 0 ? 0 : (d > K ? K : d);
  return d < c ? d : c;
}
// Ring rows for K in 1..LGX_MAX_SENSOR_HISTORY: this step's raw row goes to c % K, the raw row of
// d steps ago (0 < d <= min(K, c)) is read from (c - d) % K. With d = K both are the same row: the
// caller reads before it writes.
LGX_HD int sensor_ring_write_row(int c, int K) { return (int)((unsigned)c % (unsigned)K); }
LGX_HD int sensor_ring_read_row(int c, int d, int K) { return (int)((unsigned)(c - d) % (unsigned)K); }
// The observation-noise term of one channel: u the channel's uniform, amp its amplitude (noise_vec[i],
// times the env's scale in the sensor model). Every site that forms the term calls this.
LGX_HD float obs_noise_term(float u, float amp) { return (2.0f * u - 1.0f) * amp; }
// The noise term and the bias on channel value v (the delayed raw value on a delayed sensor
// channel), in this order, each a rounding of its own. u: the channel's uniform, nv: noise_vec[i],
// scale: &obs_noise_scale[e] or NULL, bias: &obs_bias[e][i] or NULL. Unbound, scale 1 and bias 0
// give the bits of `v + (2u - 1) * nv`; a scale of exactly 0 those of add_noise = 0.
LGX_HD float sensor_noise_bias(float v, bool add_noise, float u, float nv, const float* scale, const float* bias) {
  if (add_noise) {
    const float sc = scale ? *scale : 1.0f;
    if (!scale) v = v + obs_noise_term(u, nv);
    else if (sc != 0.0f) v = v + obs_noise_term(u, nv * sc);
  }
  if (bias) {
    const float b = *bias;
    if (b != 0.0f) v = v + b;
  }
  return v;
}

// Height-scan model (lgx_buffers.scan_noise .. scan_history, include/lgx.h, ABI 17). The rule of one
// point; the HIP kernel and the host backend both call these.
// The four uniforms of block `block` of the model's own Philox stream (the env step's counter layout).
LGX_HD void scan_uniform_block(uint64_t seed, uint32_t gid, uint64_t step, int block, float* u) {
  uint32_t o[4];
  philox4x32_10(gid, (uint32_t)step, (uint32_t)block | ((uint32_t)LGX_SCAN_STREAM << 16), (uint32_t)(step >> 32),
                (uint32_t)seed, (uint32_t)(seed >> 32), o);
  u[0] = u01(o[0]); u[1] = u01(o[1]); u[2] = u01(o[2]); u[3] = u01(o[3]);
}
// Uniform `slot` of that stream: the noise of point i is slot i, its dropout draw slot
// LGX_MAX_HEIGHT_POINTS + i.
LGX_HD float scan_uniform(uint64_t seed, uint32_t gid, uint64_t step, int slot) {
  float u[4];
  scan_uniform_block(seed, gid, step, slot >> 2, u);
  const int w = slot & 3;
  return w == 0 ? u[0] : (w == 1 ? u[1] : (w == 2 ? u[2] : u[3]));
}
// The raw value of a point from the height under it.
LGX_HD float scan_raw(float root_z, float h) { return clipf(root_z - 0.3f - h, -1.0f, 1.0f); }
// Is the point lost in this step: u its dropout uniform, p the env's probability.
LGX_HD bool scan_point_lost(float u, float p) { return p > 0.0f && u < p; }
// The model of one point on v, its (delayed) raw value: noise of amplitude amp with uniform u, the
// vertical offset dz, dropout (probability p, uniform ud, fill value), in this order, each sum a
// rounding of its own, then the clip. amp = 0, dz = 0 and p = 0 return v with its bits: the clip
// is the identity on a raw value.
LGX_HD float scan_point_model(float v, float amp, float u, float dz, float p, float ud, float fill) {
  if (amp != 0.0f) v = v + obs_noise_term(u, amp);
  if (dz != 0.0f) v = v + dz;
  if (scan_point_lost(ud, p)) v = fill;
  return clipf(v, -1.0f, 1.0f);
}

// One uniform of the env step's Philox table (fill_uniforms: slot = 4 * block + word).
LGX_HD float step_uniform(uint64_t seed, uint32_t gid, uint64_t step, int slot) {
  uint32_t o[4];
  philox4x32_10(gid, (uint32_t)step, (uint32_t)(slot >> 2), (uint32_t)(step >> 32), (uint32_t)seed,
                (uint32_t)(seed >> 32), o);
  return u01(o[slot & 3]);
}

// Go2Robot._resample_commands go2.py:413-464 / LeggedRobot legged_robot.py:406-437
// R: the mutable command ranges (lgx_buffers.command_ranges, double [8]) or NULL (params' ranges)
LGX_HD void resample_commands(const lgx_task_params* Pm, const double* R, float* cmd, const float* U, int slot0,
                              const float* quat) {
  if (Pm->has_user_command) {
    for (int i = 0; i < 4; ++i) cmd[i] = Pm->user_command[i];
    return;
  }
  if (R) {
    cmd[0] = rand_range_d(R[0], R[1], U[slot0 + 0]);
    cmd[1] = rand_range_d(R[2], R[3], U[slot0 + 1]);
    if (Pm->heading_command)
      cmd[3] = rand_range_d(R[6], R[7], U[slot0 + 2]);
    else
      cmd[2] = rand_range_d(R[4], R[5], U[slot0 + 2]);
  } else {
    cmd[0] = rand_range(Pm->cmd_lin_vel_x[0], Pm->cmd_lin_vel_x[1], U[slot0 + 0]);
    cmd[1] = rand_range(Pm->cmd_lin_vel_y[0], Pm->cmd_lin_vel_y[1], U[slot0 + 1]);
    if (Pm->heading_command)
      cmd[3] = rand_range(Pm->cmd_heading[0], Pm->cmd_heading[1], U[slot0 + 2]);
    else
      cmd[2] = rand_range(Pm->cmd_ang_vel_yaw[0], Pm->cmd_ang_vel_yaw[1], U[slot0 + 2]);
  }
  float keep = (float)(nrm2(cmd[0], cmd[1]) > 0.2f);
  cmd[0] = cmd[0] * keep;
  cmd[1] = cmd[1] * keep;
  if (Pm->zero_command && U[slot0 + 3] < Pm->zero_command_prob) {
    if (Pm->task_kind == LGX_TASK_GO2) {
      cmd[0] = cmd[0] * 0.0f; cmd[1] = cmd[1] * 0.0f; cmd[2] = cmd[2] * 0.0f;
      if (Pm->heading_command) {
        const float fwd[3] = {1.f, 0.f, 0.f};
        float f[3];
        quat_apply(quat, fwd, f);
        cmd[3] = atan2f(f[1], f[0]);
      }
    } else {
      for (int i = 0; i < 4; ++i) cmd[i] = cmd[i] * 0.0f;
    }
  }
}

// The scalar head of reset_idx for env e (go2.py:207-263 / legged_robot.py:157-213) on the
// env's staged state S (root, cmd, ep): terrain-level curriculum, root state, command resample.
// U: the env's uniforms. terrain_curriculum: whether the caller lets the curriculum run.
template <class S>
LGX_HD void reset_env_head(const lgx_task_params* Pm, const lgx_buffers& B, S& s, const float* U, int e,
                           bool terrain_curriculum) {
  float* root = s.root;
  float* cmd = s.cmd;
  // terrain curriculum legged_robot.py:543-574
  if (Pm->curriculum && terrain_curriculum && B.terrain_levels) {
    float dx = root[0] - B.env_origins[e * 3 + 0], dy = root[1] - B.env_origins[e * 3 + 1];
    float dist = nrm2(dx, dy);
    int up = dist > Pm->terrain_length * Pm->promote_threshold;
    float expct = nrm2(cmd[0], cmd[1]) * Pm->max_episode_length_s;
    int down = dist < expct * Pm->demote_threshold;
    int64_t lvl = B.terrain_levels[e] + up - down;
    if (lvl >= Pm->max_terrain_level) {
      lvl = (int64_t)(U[S_TERR] * (float)Pm->max_terrain_level);
      if (lvl >= Pm->max_terrain_level) lvl = Pm->max_terrain_level - 1;
    } else if (lvl < 0) {
      lvl = 0;
    }
    B.terrain_levels[e] = lvl;
    const float* o = B.terrain_origins + ((size_t)lvl * Pm->num_terrain_cols + B.terrain_types[e]) * 3;
    for (int i = 0; i < 3; ++i) B.env_origins[e * 3 + i] = o[i];
  }
  // _reset_root_states legged_robot.py:509-532
  for (int i = 0; i < 13; ++i) root[i] = Pm->base_init_state[i];
  for (int i = 0; i < 3; ++i) root[i] = root[i] + B.env_origins[e * 3 + i];
  if (Pm->custom_origins) {
    root[0] = root[0] + rand_range(-1.0f, 1.0f, U[S_ROOT_XY + 0]);
    root[1] = root[1] + rand_range(-1.0f, 1.0f, U[S_ROOT_XY + 1]);
  }
  for (int i = 0; i < 6; ++i) root[7 + i] = rand_range(-0.5f, 0.5f, U[S_ROOT_VEL + i]);
  resample_commands(Pm, B.command_ranges, cmd, U, S_RCMD, root + 3);
  // command schedule (include/lgx.h, ABI 10): the new episode starts in the segment of step 0
  if (B.cmd_step)
    scheduled_command(cmd, B.cmd_step + (size_t)e * LGX_CMD_SEGMENTS, B.cmd_val + (size_t)e * LGX_CMD_SEGMENTS * 4, 0);
  s.ep = 0;
}

// One reward term (the `_reward_<name>` methods; ids in include/lgx.h) on a backend's env
// state S: x (Scratch), root, cmd, th, cf, lc, lch, fat, jsum.
// Side effects (kept from the reference): feet_air_time (go2.py:827-830) and the in-place
// wrap of commands[:, 3] (go2.py:744) are written back to the state.
template <class S>
LGX_HD float reward_term(const lgx_task_params* Pm, S& s, int id) {
  const Scratch& x = s.x;
  const float* root = s.root;
  float* cmd = s.cmd;
  const float* lch = s.lch;
  float* fat = s.fat;
  const int* lc = s.lc;
  float r = 0.0f;
  switch (id) {
    case LGX_REW_ACTION_RATE: return s.jsum[J_ACTION_RATE];
    case LGX_REW_ANG_VEL_XY: return sq(x.bav[0]) + sq(x.bav[1]);
    case LGX_REW_BASE_HEIGHT:
      return sq(s.jsum[J_HEIGHT] / (float)Pm->num_height_points - Pm->base_height_target);
    case LGX_REW_CALF_COLLISION:
      for (int i = 0; i < 4; ++i) { const float* c = s.cf[Pm->calf_idx[i]]; r += (float)(nrm3(c[0], c[1], c[2]) > 0.1f); }
      return r;
    case LGX_REW_CALF_POS: return s.jsum[J_CALF_POS];
    case LGX_REW_CALF_SYMMETRY: {
      const int* c = Pm->calf_joint_idx;
      return fabsf(s.th[c[0]] - s.th[c[1]]) + fabsf(s.th[c[2]] - s.th[c[3]]);
    }
    case LGX_REW_COLLISION:
      for (int i = 0; i < Pm->n_penalised; ++i) {
        const float* c = s.cf[Pm->penalised_idx[i]];
        r += (float)(nrm3(c[0], c[1], c[2]) > 0.1f);
      }
      return r;
    case LGX_REW_DELTA_TORQUES: return s.jsum[J_DELTA_TORQUES];
    case LGX_REW_DOF_ACC: return s.jsum[J_DOF_ACC];
    case LGX_REW_DOF_ERROR: return s.jsum[J_DOF_ERROR];
    case LGX_REW_DOF_POS_LIMITS: return s.jsum[J_DOF_POS_LIMITS];
    case LGX_REW_DOF_VEL: return s.jsum[J_DOF_VEL];
    case LGX_REW_DOF_VEL_LIMITS: return s.jsum[J_DOF_VEL_LIMITS];
    case LGX_REW_FEET_AIR_TIME: {
      float rew = 0.0f;
      for (int f = 0; f < Pm->num_feet; ++f) {
        int cfl = (s.cf[Pm->feet_idx[f]][2] > 1.0f) || lc[f];
        float first = (float)((fat[f] > 0.0f) && cfl);
        fat[f] = fat[f] + Pm->dt;
        rew += (fat[f] - 0.5f) * first;
      }
      rew = rew * (float)(nrm2(cmd[0], cmd[1]) > 0.1f);
      for (int f = 0; f < Pm->num_feet; ++f) {
        int cfl = (s.cf[Pm->feet_idx[f]][2] > 1.0f) || lc[f];
        fat[f] = fat[f] * (float)(!cfl);
      }
      return rew;
    }
    case LGX_REW_FEET_CONTACT_FORCES:
      for (int f = 0; f < Pm->num_feet; ++f) {
        const float* c = s.cf[Pm->feet_idx[f]];
        float v = nrm3(c[0], c[1], c[2]) - Pm->max_contact_force;
        r += v > 0.0f ? v : 0.0f;
      }
      return r;
    case LGX_REW_HEADING_ALIGNMENT: {
      const float fwd[3] = {1.f, 0.f, 0.f};
      float f[3];
      quat_apply(root + 3, fwd, f);
      float heading = atan2f(f[1], f[0]);
      float desired = 0.0f;
      if (Pm->heading_command) {
        cmd[3] = wrap_to_pi(cmd[3]);  // wrap_to_pi mutates commands[:, 3] (Q7)
        desired = cmd[3];
      }
      float err = wrap_to_pi(desired - heading);
      return sq(err) * (float)(nrm3(cmd[0], cmd[1], cmd[2]) >= 0.2f);
    }
    case LGX_REW_HIP_POS: return s.jsum[J_HIP_POS];
    case LGX_REW_JUMP_ZONE_FORWARD_VEL: {
      float fr = root[7] > 0.0f ? root[7] : 0.0f;
      return fr * (float)(x.jump > 0.0f) * (float)(nrm3(cmd[0], cmd[1], cmd[2]) >= 0.2f);
    }
    case LGX_REW_JUMP_ZONE_UPWARD_VEL: {
      float up = root[9] > 0.0f ? root[9] : 0.0f;
      return up * (float)(x.jump > 0.0f) * (float)(nrm3(cmd[0], cmd[1], cmd[2]) >= 0.2f);
    }
    case LGX_REW_LIN_VEL_Z: return sq(x.blv[2]);
    case LGX_REW_MIN_HEIGHT: {
      float ze = clipf(Pm->base_height_target - root[2], 0.0f, Pm->base_height_target);
      return ze * (float)(x.jump > 0.0f);
    }
    case LGX_REW_ORIENTATION: return sq(x.pg[0]) + sq(x.pg[1]);
    case LGX_REW_PHASE_CONTACT_MATCH: {
      float thr = 2.0f * Pm->percent_time_on_ground - 1.0f;
      float rew = 0.0f;
      for (int f = 0; f < 4; ++f) {
        int stance = sinf(6.283185307179586f * x.ph[f]) <= thr;
        rew += (x.contact[f] == stance) ? 0.25f : -0.25f;
      }
      return rew;
    }
    case LGX_REW_PHASE_FOOT_LIFTING: {
      float thr = 2.0f * Pm->percent_time_on_ground - 1.0f;
      float rew = 0.0f;
      for (int f = 0; f < 4; ++f) {
        int stance = sinf(6.283185307179586f * x.ph[f]) <= thr;
        float h = clipf(x.feet_z[f] - lch[f], 0.0f, Pm->max_foot_height);
        float nh = h / Pm->max_foot_height;
        rew += stance ? -nh : nh;
      }
      return rew / 2.0f;
    }
    case LGX_REW_REVERSE_PENALTY: return -(root[7] < 0.0f ? root[7] : 0.0f);
    case LGX_REW_STAND_STILL: return s.jsum[J_STAND_ABS] * (float)(nrm2(cmd[0], cmd[1]) < 0.1f);
    case LGX_REW_STUMBLE_CALVES: {
      int any = 0;
      for (int i = 0; i < 4; ++i) { const float* c = s.cf[Pm->calf_idx[i]]; any |= nrm2(c[0], c[1]) > 5.0f * fabsf(c[2]); }
      return (float)any;
    }
    case LGX_REW_STUMBLE_FEET: {
      int any = 0;
      for (int f = 0; f < Pm->num_feet; ++f) { const float* c = s.cf[Pm->feet_idx[f]]; any |= nrm2(c[0], c[1]) > 5.0f * fabsf(c[2]); }
      return (float)any;
    }
    case LGX_REW_THIGH_POS: return s.jsum[J_THIGH_POS];
    case LGX_REW_THIGH_SYMMETRY: {
      const int* c = Pm->thigh_joint_idx;
      return fabsf(s.th[c[0]] - s.th[c[1]]) + fabsf(s.th[c[2]] - s.th[c[3]]);
    }
    case LGX_REW_TORQUE_LIMITS: return s.jsum[J_TORQUE_LIMITS];
    case LGX_REW_TORQUES: return s.jsum[J_TORQUES];
    case LGX_REW_TRACKING_ANG_VEL: return expf(-sq(cmd[2] - x.bav[2]) / Pm->tracking_sigma);
    case LGX_REW_TRACKING_LIN_VEL: return expf(-(sq(cmd[0] - x.blv[0]) + sq(cmd[1] - x.blv[1])) / Pm->tracking_sigma);
    case LGX_REW_TRACKING_PITCH: {
      float deg = x.pitch * 57.29577951308232f;
      return expf(-sq(deg - Pm->pitch_deg_target) / Pm->tracking_sigma);
    }
    case LGX_REW_TRACKING_ROLL: {
      float deg = x.roll * 57.29577951308232f;
      return expf(-sq(deg - Pm->roll_deg_target) / Pm->tracking_sigma);
    }
    case LGX_REW_ZERO_CMD_DOF_ERROR:
      return s.jsum[J_DOF_ERROR] * (float)(nrm3(cmd[0], cmd[1], cmd[2]) < 0.2f);
    default: return 0.0f;
  }
}

// update_command_curriculum (go2.py:80-107 / legged_robot.py:580-591), the range update.
// S, Cn: sum and count of the pre-reset tracking_lin_vel episode sums (curriculum_vals) over
// the envs reset in this step. Widens command_ranges (and command_range_log) when their mean
// passes the threshold; returns whether the range changed.
LGX_HD bool curriculum_update_ranges(const lgx_task_params* Pm, const lgx_buffers& B, double S, double Cn) {
  int ch = 0;
  // torch.mean (fp32) / max_episode_length, compared in fp32 (no reset: reset_idx returns early)
  const float mean = Cn > 0.0 ? ((float)S / (float)Cn) / (float)Pm->max_episode_length : 0.f;
  if (Cn > 0.0 && mean > Pm->curriculum_threshold) {
    double* R = B.command_ranges;
    const double lo = R[0], hi = R[1], d = Pm->curriculum_delta;
    const double lo_max = Pm->curriculum_lo_free ? lo - d : Pm->curriculum_lo_max;
    const double nlo = fmin(fmax(lo - d, Pm->curriculum_lo_min), lo_max);  // np.clip
    const double nhi = fmin(fmax(hi + d, 0.0), Pm->curriculum_hi_max);
    ch = (nlo != lo) || (nhi != hi);
    R[0] = nlo;
    R[1] = nhi;
    float* L = B.command_range_log;
    if (L) {
      if (Pm->command_curriculum == 1) { L[0] = (float)nhi; L[1] = (float)nlo; L[2] = (float)R[3]; L[3] = (float)R[5]; }
      else { L[0] = (float)nhi; L[1] = (float)R[3]; L[2] = (float)R[5]; }
    }
  }
  return ch != 0;
}

// After a range change, env e (reset in this step): its commands are resampled again from the
// same uniforms with the new range (reset_idx resamples after the curriculum, go2.py:222-230)
// and the command entries of its observation rows are rewritten (a reset env's history is zero
// in obs and all copies of the current observation in obs_history, go2.py:570-574).
LGX_HD void curriculum_rewrite_env(const lgx_task_params* Pm, const lgx_buffers& B, uint64_t seed, uint64_t step,
                                   int e) {
  const bool go2 = Pm->task_kind == LGX_TASK_GO2;
  const int Pp = Pm->num_proprio, H = Pm->history_len, c0 = go2 ? 5 : 9;
  const float co = Pm->clip_obs;
  const uint32_t gid = (uint32_t)(Pm->env_id_offset + e);
  float U[4];  // the reset's command draws (slots S_RCMD..+3)
  for (int k = 0; k < 4; ++k) U[k] = step_uniform(seed, gid, step, S_RCMD + k);
  float cmd[4];
  for (int k = 0; k < 4; ++k) cmd[k] = B.commands[e * 4 + k];
  const float* quat = B.root_states + (size_t)e * 13 + 3;
  resample_commands(Pm, B.command_ranges, cmd, U, 0, quat);
  if (B.cmd_step)  // command schedule (ABI 10): a reset env is in the segment of step 0
    scheduled_command(cmd, B.cmd_step + (size_t)e * LGX_CMD_SEGMENTS, B.cmd_val + (size_t)e * LGX_CMD_SEGMENTS * 4, 0);
  for (int k = 0; k < 4; ++k) B.commands[e * 4 + k] = cmd[k];
  float* obs = B.obs + (size_t)e * Pm->num_obs;
  float* cr = (go2 && B.critic) ? B.critic + (size_t)e * Pm->num_critic : nullptr;
  float* hist = B.obs_history + (size_t)e * H * Pp;
  for (int j = 0; j < 3; ++j) {
    const int i = c0 + j;
    float v = cmd[j] * Pm->commands_scale[j];
    // the sensor model's noise scale and bias (ABI 15; commands are no sensor channels: no latency)
    v = sensor_noise_bias(v, Pm->add_noise != 0, Pm->add_noise ? step_uniform(seed, gid, step, S_NOISE + i) : 0.f,
                          Pm->noise_vec[i], B.obs_noise_scale ? B.obs_noise_scale + e : nullptr,
                          B.obs_bias ? B.obs_bias + (size_t)e * Pp + i : nullptr);
    const float vc = clipf(v, -co, co);
    obs[H * Pp + i] = vc;
    if (cr) cr[H * Pp + i] = vc;
    for (int t = 0; t < H; ++t) hist[t * Pp + i] = v;  // reset env: every history row = current obs
  }
}

}  // namespace lgx
