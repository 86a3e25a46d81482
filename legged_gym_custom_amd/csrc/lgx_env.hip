// lgx_env.hip — MI355X (gfx950) env-step kernels behind include/lgx.h.
//
// One wavefront (64 lanes) per environment, or two environments per wavefront (32 lanes each:
// the default on the plane with an even env count, see launch_step); the env's state lives in
// LDS for the whole step (decimation physics substeps + post-physics), so HBM sees each per-env
// row once in and once out, coalesced (rows are env-major, lanes sweep a row).
//
// Physics (replaces PhysX `gym.simulate`, legged_robot.py:79-85; spec in DESIGN.md):
//   lanes 0..11  PD torques (legged_robot.py:440-478)
//   lanes 0..12  kinematics, one lane per joint (lane 12 the base), parent state passed down
//                the chain by DPP; per-link COM wrench and the base sums about p0
//   lanes 0..39  mass matrix [A B; Bᵀ D] factored lane-parallel: joint bias and coupling,
//                leg blocks D_l, X = B D⁻¹, the 21 Schur sums, S⁻¹ by a register Cholesky
//   lanes 0..63  contact candidates (one sphere centre per lane) -> ballot-compacted rows
//   lanes 0..R-1 one constraint row each: Jacobian row, M⁻¹Jᵀ column (Schur solve), A_rr,
//                then projected Gauss-Seidel on A = J M⁻¹ Jᵀ (lane r holds row r's velocity
//                and impulse; A stored in LDS, or formed per row for a fallen robot's rows)
// Post-physics (Go2Robot.post_physics_step go2.py:345-387, LeggedRobot legged_robot.py:
//   103-138): uniform scalar control flow per env; vector outputs written lane-parallel.
// The scalar code with no lane index in it (vector math, Philox, constants and slots, reward
// terms, command resampling, the heads of reset and of the command curriculum) is shared with
// the host backend: lgx_env_common.h.
#include <hip/hip_runtime.h>
#include "lgx_knobs.h"
#include <math.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/lgx.h"
#include "lgx_device.h"
#include "lgx_env_common.h"
#include "lgx_host.h"

namespace lgx {

// LDS arena (dynamic shared memory, sized per launch by arena_floats) time-shared by phase:
//   dynamics   Fw, Nw [NL][3], Dl [4][6], tot [16]
//   rows       ZG [MAXR][RW] at 0: z_r = S⁻¹ (J_b − X_l J_l) (6) | g_r = D_l⁻¹ J_l (3);
//              J9 [MAXR][RW] at MAXR*RW: sparse row r = [base part (6) | the 3 joints of leg
//              rleg[r]]; once J9 is in registers, the same region holds A = J M⁻¹ Jᵀ: square
//              [n][n] for n <= ASQ rows, packed lower triangle for ASQ < n <= AMAX (see substep)
//   post       U [4 rng_blocks] | cur [P] | hist [H*P] | heights [Hp] (stg_* below)
// Go2 needs 1116 floats (the rows), ANYmal's post-physics staging 1,924.
// Rows per env step: p50 9, p99 15, max 27 (tools/phase_clock.py, r02). The launch time is
// the slowest wave's, so the rare env above ASQ rows must not fall to the velocity-space sweep
// (a launch with one such env took 25-65 % longer): up to AMAX rows A is kept as a packed
// lower triangle in the same LDS.
constexpr int ASQ = 24;   // square A up to here
constexpr int AMAX = 33;  // packed-triangle A up to here (33 * 34 / 2 = 561 <= 24 * 24)
constexpr int RW = 9;     // sparse row width
constexpr int A_FLOATS = ASQ * ASQ > AMAX * (AMAX + 1) / 2 ? ASQ * ASQ : AMAX * (AMAX + 1) / 2;
constexpr int J9_FLOATS = MAXR * RW > A_FLOATS ? MAXR * RW : A_FLOATS;
constexpr int ROWS_FLOATS = MAXR * RW + J9_FLOATS;
extern __shared__ float lgx_dyn[];
struct DynTemps {
  float Fw[NL][3], Nw[NL][3];  // per-link COM wrench (bias)
  float Dl[4][6];              // leg blocks of the joint-space inertia (xx yy zz xy xz yz)
  float tot[16];               // base sums about p0: m, h(3), Ip(6), F(3), N(3)
  float Sp[21];                // Σ_j X_j B_jᵀ, packed lower
};
static_assert(sizeof(DynTemps) <= ROWS_FLOATS * sizeof(float), "dynamics temporaries fit the arena");
// Each env owns one arena (A below: lgx_dyn, or lgx_dyn + arena_floats for the second env of a
// paired wave, see env_step_kernel)
LGX_DEV DynTemps& dtmp(float* A) { return *reinterpret_cast<DynTemps*>(A); }
LGX_DEV float* stg_U(float* A) { return A; }
LGX_DEV float* stg_cur(float* A, const lgx_task_params* Pm) { return A + 4 * rng_blocks(Pm); }
// The old observation history is staged in LDS when it is short (Go2: 10 x 52 = 520); a long
// one (ANYmal: 5 x 235 = 1175, 4.7 KB) is shifted in place in HBM instead (post-physics below),
// which keeps ANYmal's arena at the Go2 size: 9.9 KB of LDS per env, 16 envs per CU.
constexpr int HIST_LDS_MAX = 640;
__host__ __device__ inline bool hist_in_lds(const lgx_task_params* Pm) {
  return Pm->history_len * Pm->num_proprio <= HIST_LDS_MAX || Pm->num_proprio < 64;
}
LGX_DEV float* stg_hist(float* A, const lgx_task_params* Pm) { return stg_cur(A, Pm) + Pm->num_proprio; }
LGX_DEV float* stg_heights(float* A, const lgx_task_params* Pm) {
  return stg_hist(A, Pm) + (hist_in_lds(Pm) ? Pm->history_len * Pm->num_proprio : 0);
}
__host__ __device__ inline int64_t arena_floats(const lgx_task_params& p) {
  const int64_t post = 4 * (9 + (p.num_proprio + 3) / 4) + p.num_proprio +
                       (hist_in_lds(&p) ? (int64_t)p.history_len * p.num_proprio : 0) + p.num_height_points;
  return post > ROWS_FLOATS ? post : ROWS_FLOATS;
}

constexpr int FRC_ON = 0, FRC_F = 1, FRC_PT = 4;  // the external force's words of Sh::rterm
struct Sh {
  // --- post-physics per-env scalars (written by lane 0, read by all lanes)
  Scratch x;
  float root[13], cmd[4], fat[4], lch[4];
  int lc[4];
  // rterm: the reward terms, first written after the physics. During the physics its first words
  // hold the external force (include/lgx.h, ABI 16) that the FORCE instances stage once per step and
  // the substeps read: [FRC_ON] 1 when it acts in this step, else 0, [FRC_F..+2] the world vector,
  // [FRC_PT..+2] the application point in the base link frame. So Sh keeps its layout and the
  // instances without the force their code.
  float rterm[64];
  float jsum[16];  // per-env joint / height-point sums the reward terms share (joint_sums)
  // post-physics inputs read at kernel start (their HBM latency hides behind the physics)
  long long ep_prev;
  int lc_prev[LGX_MAX_FEET];
  float lch_prev[LGX_MAX_FEET], fat_prev[LGX_MAX_FEET], jump_prev;
  float la_prev[NJ], lt_prev[NJ];     // last_actions / last_torques (reward joint sums)
  float es[LGX_MAX_REWARDS + 4];      // episode_sums row (updated by this step's terms)
  float fric;                         // raw friction coefficient (privileged obs)
  long long ep;
  int reset, tout;
  int blew;  // this step's physics went non-finite (NaN/Inf guard; the env is reset)
  // --- physics state (base velocity kept as the ORIGIN velocity inside the step)
  float qb[4], pb[3], vo[3], wb[3];
  float th[NJ], thd[NJ], tau[NJ], act[NJ], kpm[NJ], kdm[NJ], ldv[NJ];
  float madd, cadd[3], mu;
  // --- kinematics per dynamic link
  float R[NL][9], P[NL][3], Ax[NL][3], W[NL][3], V[NL][3], C[NL][3], I[NL][6], m[NL];
  // --- dynamics
  float Bc[NJ][6], Dinv[4][6], X[NJ][6], Sinv[6][6], us[NU], up[NU];
  // --- constraints (J, M⁻¹Jᵀ and A live in the arena below)
  float Arr[MAXR], tgt[MAXR], lam[MAXR];
  int rleg[MAXR];
  int cbody[MAXC];
  float cn[MAXC][3];  // contact normals (terrain); tangents follow from contact_tangents
  int nrows, nlim, ncon;
  float cf[LGX_MAX_BODIES][3];
  float rbz[LGX_MAX_BODIES];
#ifdef LGX_PHASE_CLOCK
  uint64_t phlast;
  uint32_t phacc[20];
#endif
};

// ---- per-phase cycle counters (dev builds only: -DLGX_PHASE_CLOCK, tools/phase_clock.py).
// Lane 0 accumulates s_memtime deltas per phase in LDS; the kernel's end writes them to
// g_phase_out[env][phase]. Compiled out of the product library.
#ifdef LGX_PHASE_CLOCK
constexpr int NPH = 20;  // 16 phases + [16] max constraint rows, [17] wide-path substeps, [18] HW_ID, [19] XCC_ID
__device__ uint32_t* g_phase_out = nullptr;
#define PH(k)                                              \
  do {                                                     \
    if (lane == 0) {                                       \
      const uint64_t _t = clock64();                       \
      s.phacc[k] += (uint32_t)(_t - s.phlast);             \
      s.phlast = _t;                                       \
    }                                                      \
  } while (0)
#else
#define PH(k) \
  do {        \
  } while (0)
#endif

// ============================================================== physics helpers
#pragma clang fp contract(fast)

// a pointer the compiler must treat as changed here (defeats loop-invariant hoisting)
template <class T>
LGX_DEV const T* opaque(const T* p) {
  __asm__ volatile("" : "+s"(p));
  return p;
}

// XCD-aware env order. The hardware deals consecutive blocks to the 8 XCDs in turn, and env e's
// rows ([N,13] root state, [N,24] dof state, ...) share 128-B lines with env e +- 1's, so neighbouring
// envs are given blocks of the same XCD (one L2 fetches the shared line once): XCD x = b % 8 runs
// the contiguous env range [x*q + min(x, r), ...) of q + (x < r) envs (N = 8q + r) — a bijection
// of [0, N).
LGX_DEV int env_of_block(int b, int n) {
  const int q = n >> 3, r = n & 7, x = b & 7, j = b >> 3;
  return x * q + min(x, r) + j;
}

#ifndef LGX_ROW_PRIO
#define LGX_ROW_PRIO 9  // 0: no priority
#endif
#ifndef LGX_SLOT_PRIO
#define LGX_SLOT_PRIO 0  // 1: issue priority by the wave's slot on its SIMD (see env_step_kernel)
#endif

// the wave's slot on its SIMD (HW_ID wave_id field)
LGX_DEV int wave_slot() { return __builtin_amdgcn_s_getreg(4 | (3 << 11)) & 15; }
// s_setprio(p) for a runtime p in 0..3
LGX_DEV void set_prio(int p) {
  if (p >= 3) __builtin_amdgcn_s_setprio(3);
  else if (p == 2) __builtin_amdgcn_s_setprio(2);
  else if (p == 1) __builtin_amdgcn_s_setprio(1);
  else __builtin_amdgcn_s_setprio(0);
}

LGX_DEV int opaque_lane(int v) {
  __asm__ volatile("" : "+v"(v));
  return v;
}

// ---- lane groups. An env owns WL consecutive lanes of its wave: WL = 64 (one env per wave) or
// WL = 32 (two envs per wave, lanes 0..31 and 32..63: the phases that use a dozen to thirty
// lanes of an env then do two envs' work per instruction). The physics and post-physics
// functions below take `lane` = the lane within the group and the group's own Sh / arena; the
// helpers here are the cross-lane operations made group-local. (DPP row operations act on
// 16-lane rows and are group-local as they are.)
template <int WL>
LGX_DEV int grp_of_lane() {
  if constexpr (WL == 64) return 0;
  else return (int)(__lane_id() >> 5);
}
// this group's ballot, bit i = group lane i
template <int WL>
LGX_DEV uint64_t gballot(bool p) {
  const uint64_t m = __ballot(p);
  if constexpr (WL == 64) return m;
  else return (__lane_id() >> 5) ? (m >> 32) : (m & 0xffffffffull);
}
LGX_DEV float rdl(float v, int l) { return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), l)); }
LGX_DEV int rdl(int v, int l) { return __builtin_amdgcn_readlane(v, l); }
// v of group lane r0 (group 0) / r1 (group 1), in every lane of the group (r0, r1 wave-uniform)
template <int WL>
LGX_DEV float gbcast(float v, int r0, int r1) {
  if constexpr (WL == 64) {
    return rdl(v, r0);
  } else {
    const float a = rdl(v, r0), b = rdl(v, 32 + r1);
    return (__lane_id() >> 5) ? b : a;
  }
}
template <int WL>
LGX_DEV float gbcast(float v, int r) { return gbcast<WL>(v, r, r); }
// a * b for a, b < 2^24 as one full-rate v_mul_u32_u24 (the compiler otherwise folds small
// index products into 64-bit multiply-adds)
LGX_DEV int mul24(int a, int b) {
  int r;
  __asm__("v_mul_u32_u24 %0, %1, %2" : "=v"(r) : "v"(a), "v"(b));
  return r;
}
// a group-uniform int of group 0 / group 1 as wave-uniform scalars
template <int WL>
LGX_DEV int gval(int v, int g) {
  if constexpr (WL == 64) return __builtin_amdgcn_readfirstlane(v);
  else return rdl(v, 32 * g);
}
// the largest of the groups' values of a group-uniform int (a wave-uniform loop bound)
template <int WL>
LGX_DEV int gmax(int v) {
  if constexpr (WL == 64) return __builtin_amdgcn_readfirstlane(v);
  else return max(rdl(v, 0), rdl(v, 32));
}
// sum over group lanes 0..15 (the group's first DPP row), returned to every lane of the group;
// lanes 0..15 of the group must be active
template <int WL>
LGX_DEV float grow_sum16(float x) {
  x += dpp_shr_t<0x111>(x);
  x += dpp_shr_t<0x112>(x);
  x += dpp_shr_t<0x114>(x);
  x += dpp_shr_t<0x118>(x);
  return gbcast<WL>(x, 15);
}

// lane i receives lane i-1's value (DPP row_shr:1; lanes 0..15 form one row)
LGX_DEV float from_prev_lane(float x) { return dpp_shr_t<0x111>(x); }

// Forward kinematics, velocities and bias accelerations, one lane per link: lane j < 12
// is joint j / link j+1 (leg j/3, chain position j%3), lane 12 the base. A chain is three
// deep: each of three rounds composes every lane with its parent's world state, then the
// parent state moves one lane down the chain by DPP, so no lane waits on LDS. Writes the
// link arrays the later phases read (R, P, Ax, W, V, C, I, m). With BIAS, the same lanes
// also form the per-link COM wrench (Fw, Nw) and return the 16 base sums about p0 (mass,
// first moment, inertia, wrench), reduced across lanes 0..15 by DPP (see dynamics).
// FORCE (with BIAS): the external force of ABI 16 on the base link, staged in s.rterm (FRC_*).
template <bool BIAS, bool FORCE = false>
LGX_DEV void kinematics(Sh& s, float* A, const lgx_model* M, const lgx_task_params* Pm, int lane) {
  const int j = lane < NJ ? lane : NJ - 1;
  const bool base = lane == NJ;  // the base rides the chain as a fixed joint at the root
  const int a = base ? 0 : j % 3;
  const int k = base ? 0 : j + 1;
  // per-lane model constants (vector loads, L1-resident); identity joint for the base lane
  const float bm = base ? 0.f : 1.f;
  const f3 orig = ld3(M->joint_origin[j + 1]) * bm, al = ld3(M->joint_axis[j + 1]) * bm;
  float Rj[9];
  {
    const float* Rjp = M->joint_rot[j + 1];
#pragma unroll
    for (int q = 0; q < 9; ++q) Rj[q] = base ? ((q & 3) == 0 ? 1.f : 0.f) : Rjp[q];
  }
  // local rotation of joint j: joint frame, then the axis-angle rotation
  const float th = base ? 0.f : s.th[j], thd = base ? 0.f : s.thd[j];
  float Rl[9];
  {
    const float ct = cosf(th), st = sinf(th), t1 = 1.f - ct;
    const float Ra[9] = {t1 * al.x * al.x + ct, t1 * al.x * al.y - st * al.z, t1 * al.x * al.z + st * al.y,
                         t1 * al.x * al.y + st * al.z, t1 * al.y * al.y + ct, t1 * al.y * al.z - st * al.x,
                         t1 * al.x * al.z - st * al.y, t1 * al.y * al.z + st * al.x, t1 * al.z * al.z + ct};
    mm(Rj, Ra, Rl);
  }
  const f3 axl = mv(Rj, al);
  // parent state, initially the base (uniform)
  float Rp[9];
  quat_to_R(s.qb, Rp);
  f3 Pp = ld3(s.pb), Wp = ld3(s.wb), Vp = ld3(s.vo), Alp = mk(0.f, 0.f, 0.f), Aop = mk(0.f, 0.f, 0.f);
  float R[9];
  f3 P, ax, W, V, Al, Ao;
#pragma unroll 1
  for (int d = 0; d < 3; ++d) {
    const f3 o = mv(Rp, orig);
    ax = mv(Rp, axl);
    mm(Rp, Rl, R);
    P = Pp + o;
    const f3 wa = ax * thd;
    W = Wp + wa;
    if constexpr (BIAS) {
      Al = Alp + cross(Wp, wa);
      Ao = Aop + cross(Alp, o) + cross(Wp, cross(Wp, o));
    } else {
      V = Vp + cross(Wp, o);
    }
    if (d < 2) {
      const bool take = a == d + 1;
#pragma unroll
      for (int q = 0; q < 9; ++q) {
        const float v = from_prev_lane(R[q]);
        Rp[q] = take ? v : Rp[q];
      }
#define LGX_PASS(dst, src)                                                                          \
  {                                                                                                 \
    const float vx = from_prev_lane(src.x), vy = from_prev_lane(src.y), vz = from_prev_lane(src.z); \
    dst.x = take ? vx : dst.x;                                                                      \
    dst.y = take ? vy : dst.y;                                                                      \
    dst.z = take ? vz : dst.z;                                                                      \
  }
      LGX_PASS(Pp, P)
      LGX_PASS(Wp, W)
      if constexpr (BIAS) {
        LGX_PASS(Alp, Al)
        LGX_PASS(Aop, Ao)
      } else {
        LGX_PASS(Vp, V)
      }
#undef LGX_PASS
    }
  }
  const float* clp = M->link_com[k];
  const float cb = base ? 1.f : 0.f;
  const f3 cl = mk(clp[0] + cb * s.cadd[0], clp[1] + cb * s.cadd[1], clp[2] + cb * s.cadd[2]);
  const f3 C = P + mv(R, cl);
  if (lane <= NJ) {
#pragma unroll
    for (int q = 0; q < 9; ++q) s.R[k][q] = R[q];
    st3(s.P[k], P);
    st3(s.Ax[k], ax);
    st3(s.W[k], W);
    st3(s.C[k], C);
    if constexpr (!BIAS) st3(s.V[k], V);
  }
  if constexpr (BIAS) {
    const float m = M->link_mass[k] + cb * s.madd;
    // world inertia about the COM: R I Rᵀ
    float Iw[6];
    {
      const float* In = M->link_inertia[k];
      const float Il[9] = {In[0], In[3], In[4], In[3], In[1], In[5], In[4], In[5], In[2]};
      float T[9];
      mm(R, Il, T);
      Iw[0] = T[0] * R[0] + T[1] * R[1] + T[2] * R[2];
      Iw[1] = T[3] * R[3] + T[4] * R[4] + T[5] * R[5];
      Iw[2] = T[6] * R[6] + T[7] * R[7] + T[8] * R[8];
      Iw[3] = T[0] * R[3] + T[1] * R[4] + T[2] * R[5];
      Iw[4] = T[0] * R[6] + T[1] * R[7] + T[2] * R[8];
      Iw[5] = T[3] * R[6] + T[4] * R[7] + T[5] * R[8];
    }
    const f3 g = ld3(Pm->gravity);
    const f3 rl = C - P;
    const f3 acc = Ao + cross(Al, rl) + cross(W, cross(W, rl));
    f3 F = (acc - g) * m;
    f3 N = symv(Iw, Al) + cross(W, symv(Iw, W));
    // external force (include/lgx.h, ABI 16): on the base link, at a = P0 + R0 * point
    if constexpr (FORCE) {
      if (base && s.rterm[FRC_ON] != 0.f) {
        const f3 f = ld3(s.rterm + FRC_F);
        F = F - f;
        N = N - cross(P + mv(R, ld3(s.rterm + FRC_PT)) - C, f);
      }
    }
    if (lane <= NJ) {
#pragma unroll
      for (int q = 0; q < 6; ++q) s.I[k][q] = Iw[q];
      s.m[k] = m;
      st3(dtmp(A).Fw[k], F);
      st3(dtmp(A).Nw[k], N);
    }
    // the 16 base sums about p0, reduced over lanes 0..15 (row 0) by a DPP scan whose
    // total lands on lane 15
    const f3 r = C - ld3(s.pb);
    const float rr = dot(r, r);
    const f3 Nt = cross(r, F) + N;
    const float on = lane <= NJ ? 1.f : 0.f;
    const float rd[16] = {m, m * r.x, m * r.y, m * r.z,
                          Iw[0] + m * (rr - r.x * r.x), Iw[1] + m * (rr - r.y * r.y), Iw[2] + m * (rr - r.z * r.z),
                          Iw[3] - m * r.x * r.y, Iw[4] - m * r.x * r.z, Iw[5] - m * r.y * r.z,
                          F.x, F.y, F.z, Nt.x, Nt.y, Nt.z};
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      float x = rd[q] * on;
      x += dpp_shr_t<0x111>(x);
      x += dpp_shr_t<0x112>(x);
      x += dpp_shr_t<0x114>(x);
      x += dpp_shr_t<0x118>(x);
      if (lane == 15) dtmp(A).tot[q] = x;
    }
  }
  __syncthreads();
}

// Mass matrix M = [A B; Bᵀ D] over u = [base origin velocity, ω | 12 joint rates] (D block
// diagonal over the 4 chains) and bias h, factored so that every later product with M⁻¹ is
// a short lane-parallel chain instead of one lane's serial solve:
//   X = B D⁻¹ (s.X[j][r] = X[r][j]),  S = A − X Bᵀ (base Schur complement),  S⁻¹ (s.Sinv)
//   M⁻¹ f = [z ; D⁻¹ f_J − Xᵀ z]  with  z = S⁻¹ (f_B − X f_J)
//   J M⁻¹ Jᵀ = y_rᵀ S⁻¹ y_s + [leg_r = leg_s] J_r,Jᵀ D_l⁻¹ J_s,J  with  y = J_B − X J_J
// Lanes:
//   D1 (in kinematics<true>) per-link COM wrench; the 16 base sums about p0 by DPP
//   D2 lanes 0..11  joint bias h_j and coupling column B_j;  lanes 8..31 leg block D_l
//   D3 lanes 0..11  D_l⁻¹ (row a), X_j; the 21 Schur sums by DPP; every lane factors S in
//                   registers (Cholesky); lanes 0..5 write column `lane` of S⁻¹
struct DynOut {
  float hb[6];    // base bias (uniform)
  float hj;       // lane j < 12: joint bias
  float xj[6];    // lane j < 12: X_j
  float dinv[3];  // lane j < 12: row a of D_l⁻¹
};

LGX_DEV void dynamics(Sh& s, float* A, int lane, DynOut& o) {
  const f3 p0 = ld3(s.P[0]);
  const float* tot = dtmp(A).tot;
  const int j = lane < NJ ? lane : NJ - 1, l = j / 3, a = j % 3;
  if (lane < NJ) {  // ---- D2a: joint j (leg l, chain position a)
    const int kj = 1 + j;
    const f3 ax = ld3(s.Ax[kj]), pj = ld3(s.P[kj]);
    f3 acc = mk(0, 0, 0), hl = mk(0, 0, 0), bang = mk(0, 0, 0);
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      if (i < a) continue;
      const int k = 1 + 3 * l + i;
      const f3 c = ld3(s.C[k]);
      const f3 d = c - pj;
      const float m = s.m[k];
      acc = acc + cross(d, ld3(dtmp(A).Fw[k])) + ld3(dtmp(A).Nw[k]);
      hl = hl + d * m;
      bang = bang + cross(c - p0, cross(ax, d)) * m + symv(s.I[k], ax);
    }
    o.hj = dot(ax, acc);
    const f3 blin = cross(ax, hl);
    float* Bj = s.Bc[j];
    Bj[0] = blin.x; Bj[1] = blin.y; Bj[2] = blin.z; Bj[3] = bang.x; Bj[4] = bang.y; Bj[5] = bang.z;
  }
  // (the two branches run one after the other in the wave either way; lanes 8..31 keep both
  // parts within one 32-lane group)
  if (lane >= 8 && lane < 32) {  // ---- D2b: leg block entry (xx yy zz xy xz yz)
    const int q = lane - 8, lq = q / 6, e = q % 6;
    const int j1 = e < 3 ? e : (e == 5 ? 1 : 0);
    const int j2 = e < 3 ? e : (e == 3 ? 1 : 2);
    const int k1 = 1 + 3 * lq + j1, k2 = 1 + 3 * lq + j2;
    const f3 a1 = ld3(s.Ax[k1]), a2 = ld3(s.Ax[k2]), p1 = ld3(s.P[k1]), p2 = ld3(s.P[k2]);
    float acc = 0.f;
#pragma unroll
    for (int i = 0; i < 3; ++i) {
      if (i < j2) continue;
      const int k = 1 + 3 * lq + i;
      const f3 c = ld3(s.C[k]);
      acc += s.m[k] * dot(cross(a1, c - p1), cross(a2, c - p2)) + dot(a1, symv(s.I[k], a2));
    }
    dtmp(A).Dl[lq][e] = acc;
  }
  __syncthreads();
  // ---- D3
  float Di[6];
  sym3_inv(dtmp(A).Dl[l], Di);
#pragma unroll
  for (int c = 0; c < 3; ++c) o.dinv[c] = sym3(Di, a, c);
  if (lane < NJ && a == 0) {
#pragma unroll
    for (int q = 0; q < 6; ++q) s.Dinv[l][q] = Di[q];
  }
  float bj[6];
  {
    const float* B0 = s.Bc[3 * l];
    const float* B1 = s.Bc[3 * l + 1];
    const float* B2 = s.Bc[3 * l + 2];
#pragma unroll
    for (int r = 0; r < 6; ++r) {
      const float b0 = B0[r], b1 = B1[r], b2 = B2[r];
      o.xj[r] = o.dinv[0] * b0 + o.dinv[1] * b1 + o.dinv[2] * b2;
      bj[r] = a == 0 ? b0 : (a == 1 ? b1 : b2);
    }
  }
  if (lane < NJ) {
#pragma unroll
    for (int r = 0; r < 6; ++r) s.X[j][r] = o.xj[r];
  }
  // the 21 Schur sums Σ_j X_j[r] B_j[c] (packed lower), one lane each over the 12 joints
  __syncthreads();
  if (lane < 21) {
    const int q = lane;
    const int r = (q >= 1) + (q >= 3) + (q >= 6) + (q >= 10) + (q >= 15), c = q - r * (r + 1) / 2;
    float acc = 0.f;
#pragma unroll
    for (int jj = 0; jj < NJ; ++jj) acc += s.X[jj][r] * s.Bc[jj][c];
    dtmp(A).Sp[q] = acc;
  }
  __syncthreads();
  // S = A_bb − Σ_j X_j B_jᵀ; A_bb = [[M I, −[H]x], [[H]x, Ip]] (base origin velocity, ω),
  // [H]x = [[0,−Hz,Hy],[Hz,0,−Hx],[−Hy,Hx,0]]
  const float Mt = tot[0], Hx = tot[1], Hy = tot[2], Hz = tot[3];
  const float Ab[21] = {Mt, 0.f, Mt, 0.f, 0.f, Mt, 0.f, -Hz, Hy, tot[4], Hz, 0.f, -Hx, tot[7], tot[5],
                        -Hy, Hx, 0.f, tot[8], tot[9], tot[6]};
  float L[21];
#pragma unroll
  for (int q = 0; q < 21; ++q) L[q] = Ab[q] - dtmp(A).Sp[q];
  float inv[6];
#pragma unroll
  for (int c = 0; c < 6; ++c) {
    float d = L[pk(c, c)];
#pragma unroll
    for (int k = 0; k < c; ++k) d -= L[pk(c, k)] * L[pk(c, k)];
    const float lcc = sqrtf(fmaxf(d, 1e-12f));
    inv[c] = 1.0f / lcc;
#pragma unroll
    for (int r = c + 1; r < 6; ++r) {
      float v = L[pk(r, c)];
#pragma unroll
      for (int k = 0; k < c; ++k) v -= L[pk(r, k)] * L[pk(c, k)];
      L[pk(r, c)] = v * inv[c];
    }
  }
  // column `lane` of S⁻¹ = L⁻ᵀ L⁻¹ e_lane
  float x[6];
#pragma unroll
  for (int r = 0; r < 6; ++r) {
    float t = lane == r ? 1.f : 0.f;
#pragma unroll
    for (int k = 0; k < r; ++k) t -= L[pk(r, k)] * x[k];
    x[r] = t * inv[r];
  }
#pragma unroll
  for (int r = 5; r >= 0; --r) {
    float t = x[r];
#pragma unroll
    for (int k = r + 1; k < 6; ++k) t -= L[pk(k, r)] * x[k];
    x[r] = t * inv[r];
  }
  if (lane < 6) {
#pragma unroll
    for (int r = 0; r < 6; ++r) s.Sinv[lane][r] = x[r];
  }
#pragma unroll
  for (int q = 0; q < 6; ++q) o.hb[q] = tot[10 + q];
}

// ---- terrain contact (heightfield / trimesh)
// The reference collides against the triangle mesh convert_heightfield_to_trimesh builds
// (terrain_utils.py:382-465, legged_robot.py:788-802) or the PhysX heightfield
// (legged_robot.py:768-786). The mesh is never materialised: vertex (i, j) sits at
// ((i + dx) hs, (j + dy) hs, h vs) - border, where h (int16) and the slope-threshold
// shift (dx, dy in {-1, 0, 1}: steep steps become vertical walls) are packed in one 32-bit
// word per vertex (B.terrain_mesh, legged_gym_custom_amd/utils/terrain_utils.pack_mesh).
// Cell (i, j) holds the two triangles (v00, v11, v01), (v00, v10, v11). One lane queries
// one contact sphere: the closest mesh point over the cells whose (shifted) triangles can
// reach it, inside/outside from the surface height under the centre.
struct TerrainHit {
  float depth;  // sphere penetration (> 0: overlapping)
  f3 n;         // unit normal, terrain -> sphere
};

// The trimesh contact query (closest point over the triangles of the cells a +-1 wall shift can
// reach; the host backend's / oracle's terrain_contact state it serially) for every contact
// candidate of the wave at once, the work spread over lanes:
// each candidate lane (cand) bounds its cell range, drops out when its sphere is above every
// vertex the range can reach (a conservative block maximum packed in the mesh words' bits
// 20-31, utils/terrain_utils.pack_mesh: such a sphere is farther than r + contact_margin from
// the surface, so it forms no row either way), and the remaining (candidate, cell) tasks run
// 64 per round, one per lane; each candidate lane then folds its tasks' closest points in the
// serial loop's (i, j, triangle) order with the same strict comparison, so the result equals
// the serial terrain_contact's exactly. One-candidate-per-lane made a wave as slow as its candidate with
// the most cells (25 cells x 2 triangles for a 0.1 m sphere) for all 22 (ANYmal) or 55 (Go2)
// lanes at once. Scratch: the LDS arena (rows are formed after detection).
constexpr int MESH_BLOCK = 8;  // vertices per block side of the packed block maxima
LGX_DEV float mesh_block_bound(uint32_t w) {  // block max height (raw units), or +inf if absent
  return (w >> 31) ? (float)((int)((w >> 20) & 0x7ffu) * 32 - 32768) : 3.0e38f;
}
template <int WL>
LGX_DEV TerrainHit terrain_contact_wave(const lgx_task_params* Pm, const lgx_buffers& B, float* A, f3 x, float r,
                                        bool cand, int lane) {
  const float hs = Pm->horizontal_scale, vs = Pm->vertical_scale;
  const int rows = Pm->hf_rows, cols = Pm->hf_cols;
  const uint32_t* mesh = B.terrain_mesh;
  int cnt = 0, ci = 0, cj = 0, i0 = 0, j0 = 0, w = 1;
  f3 p = mk(0.f, 0.f, 0.f);
  if (cand) {
    const float gx = x.x + Pm->border_size, gy = x.y + Pm->border_size;
    ci = (int)floorf(gx / hs);
    cj = (int)floorf(gy / hs);
    p = mk(gx - (float)ci * hs, gy - (float)cj * hs, x.z);
    i0 = max(ci + (int)ceilf((p.x - r) / hs) - 2, 0);
    const int i1 = min(ci + (int)floorf((p.x + r) / hs) + 1, rows - 2);
    j0 = max(cj + (int)ceilf((p.y - r) / hs) - 2, 0);
    const int j1 = min(cj + (int)floorf((p.y + r) / hs) + 1, cols - 2);
    if (i1 >= i0 && j1 >= j0) {
      w = j1 - j0 + 1;
      cnt = (i1 - i0 + 1) * w;
      if (i1 + 1 - i0 < MESH_BLOCK && j1 + 1 - j0 < MESH_BLOCK) {  // <= 2 blocks a side: the corners see them all
        const float hb = fmaxf(fmaxf(mesh_block_bound(mesh[(size_t)i0 * cols + j0]),
                                     mesh_block_bound(mesh[(size_t)i0 * cols + j1 + 1])),
                               fmaxf(mesh_block_bound(mesh[(size_t)(i1 + 1) * cols + j0]),
                                     mesh_block_bound(mesh[(size_t)(i1 + 1) * cols + j1 + 1])));
        if (hb < 1.0e38f && p.z - r - Pm->contact_margin > hb * vs + 1e-4f) cnt = 0;
      }
    }
  }
  // inclusive prefix of the task counts over the group's lanes
  int endp = cnt;
#pragma unroll
  for (int d = 1; d < WL; d <<= 1) {
    const int v = __shfl_up(endp, d, WL);
    if (lane >= d) endp += v;
  }
  const int total = __shfl(endp, WL - 1, WL);
  const int total_max = gmax<WL>(total);  // the groups' task lists run side by side
  int* const T_end = reinterpret_cast<int*>(A);
  int* const T_ci = T_end + 64;
  int* const T_cj = T_end + 128;
  int* const T_i0 = T_end + 192;
  int* const T_j0 = T_end + 256;
  int* const T_w = T_end + 320;
  float* const T_p = A + 384;        // [3][64]
  float* const R_ = A + 576;         // results [8][64]: d2, q(3), fn(3), zs
  T_end[lane] = endp; T_ci[lane] = ci; T_cj[lane] = cj; T_i0[lane] = i0; T_j0[lane] = j0; T_w[lane] = w;
  T_p[lane] = p.x; T_p[64 + lane] = p.y; T_p[128 + lane] = p.z;
  float best = 3.0e38f, zs = -3.0e38f;
  f3 q = mk(0.f, 0.f, -3.0e38f), fn = mk(0.f, 0.f, 1.f);
  const int mystart = endp - cnt;
  for (int base = 0; base < total_max; base += WL) {
    __syncthreads();  // the tables (first round) / the previous round's results are read
    const int t = base + lane;
    float td2 = 3.0e38f, tz = -3.0e38f;
    f3 tq = mk(0.f, 0.f, -3.0e38f), tfn = mk(0.f, 0.f, 1.f);
    if (t < total) {
      int lo = 0, hi = WL - 1;  // owner: the first lane whose inclusive end exceeds t
      while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (T_end[mid] > t) hi = mid; else lo = mid + 1;
      }
      const int c = lo;
      const int k = t - (c ? T_end[c - 1] : 0);  // task index within candidate c
      const int wc = T_w[c];
      const int i = T_i0[c] + k / wc, j = T_j0[c] + k % wc;
      const int cci = T_ci[c], ccj = T_cj[c];
      const f3 pc = mk(T_p[c], T_p[64 + c], T_p[128 + c]);
      const f3 v00 = mesh_vertex(mesh, cols, i, j, cci, ccj, hs, vs);
      const f3 v01 = mesh_vertex(mesh, cols, i, j + 1, cci, ccj, hs, vs);
      const f3 v10 = mesh_vertex(mesh, cols, i + 1, j, cci, ccj, hs, vs);
      const f3 v11 = mesh_vertex(mesh, cols, i + 1, j + 1, cci, ccj, hs, vs);
#pragma unroll
      for (int tri = 0; tri < 2; ++tri) {
        const f3 a = v00, b = tri == 0 ? v11 : v10, cc = tri == 0 ? v01 : v11;
        const f3 cpt = closest_on_triangle(pc, a, b, cc);
        const f3 dd = pc - cpt;
        const float d2 = dot(dd, dd);
        if (d2 < td2) { td2 = d2; tq = cpt; tfn = cross(b - a, cc - a); }
        float z;
        if (height_in_triangle(pc, a, b, cc, z)) tz = fmaxf(tz, z);
      }
    }
    R_[lane] = td2;
    R_[64 + lane] = tq.x; R_[128 + lane] = tq.y; R_[192 + lane] = tq.z;
    R_[256 + lane] = tfn.x; R_[320 + lane] = tfn.y; R_[384 + lane] = tfn.z;
    R_[448 + lane] = tz;
    __syncthreads();
    if (cnt > 0) {  // this candidate's tasks of the round, in order
      const int a0 = max(mystart, base) - base, a1 = min(endp, base + WL) - base;
      for (int sl = a0; sl < a1; ++sl) {
        const float d2 = R_[sl];
        if (d2 < best) {
          best = d2;
          q = mk(R_[64 + sl], R_[128 + sl], R_[192 + sl]);
          fn = mk(R_[256 + sl], R_[320 + sl], R_[384 + sl]);
        }
        zs = fmaxf(zs, R_[448 + sl]);
      }
    }
  }
  __syncthreads();  // the arena is the constraint rows' next
  TerrainHit h;
  if (best >= 3.0e38f) {  // culled, outside the field, or no candidate: nothing to touch
    h.depth = -3.0e38f;
    h.n = mk(0.f, 0.f, 1.f);
    return h;
  }
  const float dist = sqrtf(best);
  const bool below = p.z < zs;
  h.depth = below ? r + dist : r - dist;
  if (dist > 1e-6f) {
    h.n = (p - q) * ((below ? -1.0f : 1.0f) / dist);
  } else {
    h.n = fn * rsqrtf(fmaxf(dot(fn, fn), 1e-30f));
  }
  return h;
}

// tangent pair of a contact normal; (0,0,1) -> (1,0,0), (0,1,0) like the plane rows
// not shared with the host backend's tangents: this one uses rsqrtf(l2), the host divides by sqrtf(l2)
LGX_DEV void contact_tangents(f3 n, f3& t1, f3& t2) {
  f3 a = mk(n.z, 0.f, -n.x);  // e_y x n
  float l2 = a.x * a.x + a.z * a.z;
  if (l2 < 1e-8f) {
    a = mk(0.f, n.z, -n.y);   // n x e_x (n close to +-e_y)
    l2 = a.y * a.y + a.z * a.z;
  }
  t1 = a * rsqrtf(l2);
  t2 = cross(n, t1);
}

// ---- ANYmal series-elastic actuator net (anymal.py:71-81): 2-layer
// LSTM(2 -> 8 -> 8) step + Linear(8 -> 1), torch.nn.LSTM gate order i f g o, state [2, N*D, 8] in
// HBM (read and written once per substep). The serial per-joint statement of it is the host
// backend's sea_torque (lgx_env_host.cpp) and the oracle's (oracle/lgx_oracle.c).
// The actuator net lane-parallel over hidden units (the kernel's form): lane L serves unit
// u = L & 7 of joint j = 8 * pass + (L >> 3) — joints 0..7, then 8..11 on lanes 0..31 — and holds
// only that unit's h and c of both layers. A gate row's dot product over the 8 units of a layer
// takes the joint's other units by ds_swizzle inside the 8-lane group; every sum runs in the order
// of the serial sea_torque (the host backend's and the oracle's), so the torques are the same. Weight
// rows are lane-indexed (vector loads of the params, L1-resident): 1/8 of the per-lane work and
// transcendentals of one-joint-per-lane, and 4 state values per lane instead of 32.
// The SEA net's weight block: lgx_task_params from sea_in_scale through sea_lin_w (972 floats),
// read from its LDS arena copy.
#define SEA_OFF(f) ((int)((offsetof(lgx_task_params, f) - offsetof(lgx_task_params, sea_in_scale)) / sizeof(float)))
constexpr int SEA_WN = (int)((offsetof(lgx_task_params, sea_lin_w) + sizeof(float) * 8 -
                              offsetof(lgx_task_params, sea_in_scale)) / sizeof(float));
static_assert(SEA_WN == 972, "the SEA weight block is contiguous in lgx_task_params");
static_assert(SEA_WN <= ROWS_FLOATS, "the SEA weights fit the arena");
struct SeaW {
  float* base;  // LDS
  LGX_DEV const float* w(int off) const { return base + off; }
};
template <int K>
LGX_DEV float unit_of(float v) {  // unit K of this lane's 8-lane group
  return __int_as_float(__builtin_amdgcn_ds_swizzle(__float_as_int(v), 0x18 | (K << 5)));
}
// One LSTM cell step for unit u with the k loop outermost: the other units' values are taken by ds_swizzle
// as each k is consumed and the four gates accumulate side by side, so neither an 8-value copy of
// the units (hall / the layer-1 input) nor a gate row of weights is ever live at once. Every sum
// keeps sea_lstm_layer's order (a and b each accumulate k = 0..NIN-1 / 0..7, then (a + b_ih) + (b + b_hh)).
// XSW: the layer input is the new layer-0 h of the group's units (swizzled from xs) instead of xin.
template <int NIN, bool XSW>
LGX_DEV void sea_unit_k(const float* __restrict__ w_ih, const float* __restrict__ w_hh,
                        const float* __restrict__ b_ih, const float* __restrict__ b_hh, int u, const float* xin,
                        float xs, float hold, float& h, float& c) {
  float a[4] = {0.0f, 0.0f, 0.0f, 0.0f}, b[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
  for (int k = 0; k < NIN; ++k) {
    float xk;
    if constexpr (XSW) {
      switch (k) {
        case 0: xk = unit_of<0>(xs); break; case 1: xk = unit_of<1>(xs); break;
        case 2: xk = unit_of<2>(xs); break; case 3: xk = unit_of<3>(xs); break;
        case 4: xk = unit_of<4>(xs); break; case 5: xk = unit_of<5>(xs); break;
        case 6: xk = unit_of<6>(xs); break; default: xk = unit_of<7>(xs); break;
      }
    } else {
      xk = xin[k];
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) a[q] += w_ih[(q * 8 + u) * NIN + k] * xk;
  }
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    float hk;
    switch (k) {
      case 0: hk = unit_of<0>(hold); break; case 1: hk = unit_of<1>(hold); break;
      case 2: hk = unit_of<2>(hold); break; case 3: hk = unit_of<3>(hold); break;
      case 4: hk = unit_of<4>(hold); break; case 5: hk = unit_of<5>(hold); break;
      case 6: hk = unit_of<6>(hold); break; default: hk = unit_of<7>(hold); break;
    }
#pragma unroll
    for (int q = 0; q < 4; ++q) b[q] += w_hh[(q * 8 + u) * 8 + k] * hk;
  }
  float g4[4];
#pragma unroll
  for (int q = 0; q < 4; ++q) g4[q] = (a[q] + b_ih[q * 8 + u]) + (b[q] + b_hh[q * 8 + u]);
  // the gates on the hardware exp / rcp (v_exp_f32, v_rcp_f32, ~1 ulp each: sigmoid within
  // ~3e-7 relative, tanh(x) = 2 sigmoid(2x) - 1 within ~2e-7 absolute), ~40 instructions per
  // unit fewer than ocml expf / division / tanhf: C3 kernel 389 -> 372 us
  // (profiles/r03_sea_lds_fast.txt); ANYmal golden replay, SeaLSTM and oracle parity unchanged
  auto sg = [](float x) { return __builtin_amdgcn_rcpf(1.0f + __expf(-x)); };
  const float ig = sg(g4[0]), fg = sg(g4[1]), gg = 2.0f * sg(2.0f * g4[2]) - 1.0f, og = sg(g4[3]);
  c = fg * c + ig * gg;
  h = og * (2.0f * sg(2.0f * c) - 1.0f);
}
// Actuation latency (include/lgx.h, ABI 8), called before a substep's torques when action_delay is
// bound (a wave-uniform branch): the actuator reads s.act, so a delayed env's s.act takes the action
// of the age this substep prescribes whenever that age changes (at most twice a step): a row of
// the history, or this step's own action back from B.actions. No LDS, and nothing is kept live
// across a substep (the table and the lane are re-read here); with the feature off the cost is one
// scalar load per substep. The caller puts a barrier between this and the torques.
LGX_DEV void stage_actuator_action(Sh& s, const lgx_task_params* Pm_, const lgx_buffers& B, int e, int lane_, int sub) {
  const lgx_task_params* Pm = opaque(Pm_);
  const int AH = Pm->action_history_len, n = Pm->decimation, A = Pm->num_actions;
  const int d = action_delay_clamp(B.action_delay[e], AH, n);
  const int age = action_age(d, sub, n);  // 0..AH
  const int lane = opaque_lane(lane_);
  if (lane < A && age != (sub ? action_age(d, sub - 1, n) : 0))
    s.act[lane] = age ? B.action_history[((size_t)e * AH + (age - 1)) * A + lane] : B.actions[(size_t)e * A + lane];
}

// The same rule for the actuator net, whose unit lanes read joint j's action (of another lane): a
// delayed one straight from the history in global memory. (Staging it into s.act as above cost this
// instance a spilled VGPR on the terrain, reading it here costs the PD instances three.)
LGX_DEV float sea_action(const Sh& s, const lgx_task_params* Pm, const lgx_buffers& B, int e, int j, int sub) {
  float a = s.act[j];
  if (B.action_delay) {
    const int AH = Pm->action_history_len, n = Pm->decimation, A = Pm->num_actions;
    const int age = action_age(action_delay_clamp(B.action_delay[e], AH, n), sub, n);  // 0..AH
    if (age > 0 && j < A) a = B.action_history[((size_t)e * AH + (age - 1)) * A + j];
  }
  return a;
}

// Motor strength (include/lgx.h, ABI 8), read from global memory in the substep (a dozen lanes, L1 /
// L2 hits after the first substep) under a wave-uniform branch on the bound pointer: no LDS,
// nothing live across the substeps, and one scalar load with the feature off.
LGX_DEV float motor_strength(const lgx_task_params* Pm, const lgx_buffers& B, int e, int j) {
  return B.motor_strength ? B.motor_strength[(size_t)e * Pm->num_dof + j] : 1.0f;
}

// all 12 joints' SEA torques into s.tau (every lane of the wave takes part), one unit per lane
// over two passes. (Two units per lane in one pass measured 425-459 us vs 433 for C3's kernel,
// with 33-38 spilled VGPRs: not kept, profiles/r03_sea_spill_fix.txt.)
// inlined (54 VGPRs spill at the 4-waves-per-SIMD budget, yet C3's kernel is 589 us against 611
// as a call and 642 one joint per lane: profiles/r03_bench_anymal_c_rough_sea_waves.txt)
LGX_DEV void sea_torques_lanes(Sh& s, float* A, const lgx_task_params* Pm_, const lgx_buffers& B, int e, int lane,
                               int sub) {
  const size_t NT = (size_t)Pm_->num_envs * Pm_->num_dof;
  const int u = lane & 7;
  // The net's 972 floats (sea_in_scale .. sea_lin_w, contiguous in lgx_task_params) are copied
  // into the LDS arena, idle at the top of a substep (the previous substep's constraint rows
  // are dead, this one's not yet formed): the ~120 lane-indexed weight reads of a pass become
  // LDS reads instead of vector-memory loads (8 distinct addresses per wave instruction).
  {
    const float* src = &Pm_->sea_in_scale[0];
    for (int i = lane; i < SEA_WN; i += 64) A[i] = src[i];
    __syncthreads();
  }
#pragma unroll 1
  for (int pass = 0; pass < 2; ++pass) {
    // the weights a lane reads do not depend on the pass: an opaque table pointer per pass keeps
    // them from being hoisted out of this loop (all ~130 live at once) and spilled
    const lgx_task_params* Pm = opaque(Pm_);
    int wb = 0;  // opaque per pass, as Pm
    __asm__ volatile("" : "+s"(wb));
    const SeaW W{A + wb};
    const int j = pass * 8 + (lane >> 3);
    const bool on = j < NJ;  // pass 1: lanes 0..31 (joints 8..11); lanes 32..63 follow along
    const int jj = on ? j : NJ - 1;
    const size_t r = (size_t)e * Pm->num_dof + jj;
    float h0 = B.sea_hidden[r * 8 + u], c0 = B.sea_cell[r * 8 + u];
    float h1 = B.sea_hidden[(NT + r) * 8 + u], c1 = B.sea_cell[(NT + r) * 8 + u];
    const float in0 = (sea_action(s, Pm, B, e, jj, sub) * Pm->action_scale + Pm->default_dof_pos[jj]) - s.th[jj];
    const float x[2] = {in0 * Pm->sea_in_scale[0], s.thd[jj] * Pm->sea_in_scale[1]};
    sea_unit_k<2, false>(W.w(SEA_OFF(sea_w_ih0)), W.w(SEA_OFF(sea_w_hh0)), W.w(SEA_OFF(sea_b_ih0)),
                         W.w(SEA_OFF(sea_b_hh0)), u, x, 0.0f, h0, h0, c0);
    sea_unit_k<8, true>(W.w(SEA_OFF(sea_w_ih1)), W.w(SEA_OFF(sea_w_hh1)), W.w(SEA_OFF(sea_b_ih1)),
                        W.w(SEA_OFF(sea_b_hh1)), u, nullptr, h0, h1, h1, c1);
    if (on) {
      B.sea_hidden[r * 8 + u] = h0; B.sea_cell[r * 8 + u] = c0;
      B.sea_hidden[(NT + r) * 8 + u] = h1; B.sea_cell[(NT + r) * 8 + u] = c1;
    }
    float y = 0.0f;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      float hk;
      switch (k) {
        case 0: hk = unit_of<0>(h1); break; case 1: hk = unit_of<1>(h1); break;
        case 2: hk = unit_of<2>(h1); break; case 3: hk = unit_of<3>(h1); break;
        case 4: hk = unit_of<4>(h1); break; case 5: hk = unit_of<5>(h1); break;
        case 6: hk = unit_of<6>(h1); break; default: hk = unit_of<7>(h1); break;
      }
      y += W.w(SEA_OFF(sea_lin_w))[k] * hk;
    }
    if (on && u == 0) {
      const float t = Pm->sea_out_scale * (y + Pm->sea_lin_b);
      s.tau[j] = B.motor_strength ? motor_strength(Pm, B, e, j) * t : t;
    }
  }
}

// ---- the constraint solve of one substep for one env (oracle_physics.c steps 3-4): per row
//      (one lane each) the Schur solves, A = J M⁻¹ Jᵀ, projected Gauss-Seidel -> s.lam; z_r, g_r
//      stay in the arena (ZG) for the velocity update. Input: the rows the detection wrote (J9,
//      s.rleg, s.tgt, s.nrows / nlim / ncon). WL = the env's lanes: 64, or 32 with both envs of
//      the wave at <= 32 rows (the groups' loops then run side by side to the larger count, each
//      group predicated on its own; the broadcasts read each group's own row lane).
template <int WL>
LGX_DEV void solve_rows(Sh& s, float* A, const lgx_task_params* Pm, int lane, int nrows, int nlim, int ncon) {
  float* const ZG = A;                // [nrows][RW]: z_r (6) | g_r (3)
  float* const J9 = A + MAXR * RW;    // [nrows][RW]: J_B (6) | J of leg rleg (3)
  float* const Am = J9;               // A [nrows][nrows] (A path, after J9 is consumed)
  // ---- per row (one lane each): y = J_B − X_l J_l, z = S⁻¹ y, g = D_l⁻¹ J_l,
  //      A_rr = y·z + J_l·g, w_r = J_r u*
  const bool row_lane = lane < nrows;
  float yr[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, jlr[3] = {0.f, 0.f, 0.f}, w0 = 0.f;
  int lr = -1;
  if (row_lane) {
    const float* jr = J9 + lane * RW;
    lr = s.rleg[lane];
#pragma unroll
    for (int q = 0; q < 6; ++q) {
      yr[q] = jr[q];
      w0 += yr[q] * s.us[q];
    }
    float g[3] = {0.f, 0.f, 0.f};
    if (lr >= 0) {
#pragma unroll
      for (int c = 0; c < 3; ++c) jlr[c] = jr[6 + c];
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const float* Xc = s.X[3 * lr + c];
#pragma unroll
        for (int q = 0; q < 6; ++q) yr[q] -= Xc[q] * jlr[c];
        w0 += jlr[c] * s.us[6 + 3 * lr + c];
      }
      const float* Di = s.Dinv[lr];
      g[0] = Di[0] * jlr[0] + Di[3] * jlr[1] + Di[4] * jlr[2];
      g[1] = Di[3] * jlr[0] + Di[1] * jlr[1] + Di[5] * jlr[2];
      g[2] = Di[4] * jlr[0] + Di[5] * jlr[1] + Di[2] * jlr[2];
    }
    float* zg = ZG + lane * RW;
    float arr = jlr[0] * g[0] + jlr[1] * g[1] + jlr[2] * g[2];
#pragma unroll
    for (int q = 0; q < 6; ++q) {
      const float* Si = s.Sinv[q];
      const float zq = Si[0] * yr[0] + Si[1] * yr[1] + Si[2] * yr[2] + Si[3] * yr[3] + Si[4] * yr[4] + Si[5] * yr[5];
      zg[q] = zq;
      arr += yr[q] * zq;
    }
    zg[6] = g[0]; zg[7] = g[1]; zg[8] = g[2];
    s.Arr[lane] = arr;
    s.lam[lane] = 0.f;
  }
  __syncthreads();
  PH(6);
  // ---- A = J M⁻¹ Jᵀ: entry (q, r) = y_r·z_q + [leg_r = leg_q] J_l,r·g_q (J_l,r = 0 for rows
  //      without a leg part). Up to ASQ rows lane r stores column r of a square [q][r] image;
  //      up to AMAX the lower triangle q >= r packed at q (q + 1) / 2 + r; beyond (a fallen
  //      robot: up to 12 + 3 * MAXC rows) the PGS forms A[r][lane] from z_r, g_r (LDS) and the
  //      lane's own y, J_l (registers) each time it needs it — the same numbers, nothing stored.
  //      Two envs per wave (both <= 32 rows): each group its own form, read through a
  //      branch-free per-lane index (arow_mix below).
  const int NRm = gmax<WL>(nrows);
  const bool tri = nrows > ASQ, stored = nrows <= AMAX;
  if (stored && row_lane) {
#pragma unroll 4
    for (int q = 0; q < NRm; ++q) {
      if (q < nrows) {
        const float* zg = ZG + q * RW;
        const float v = yr[0] * zg[0] + yr[1] * zg[1] + yr[2] * zg[2] + yr[3] * zg[3] + yr[4] * zg[4] + yr[5] * zg[5];
        const float vl = jlr[0] * zg[6] + jlr[1] * zg[7] + jlr[2] * zg[8];
        const float a = v + (s.rleg[q] == lr ? vl : 0.f);
        if (!tri) Am[q * nrows + lane] = a;
        else if (q >= lane) Am[q * (q + 1) / 2 + lane] = a;
      }
    }
  }
  __syncthreads();
  PH(7);
  // ---- projected Gauss-Seidel on A (oracle_physics.c step 4). Rows are [nlim joint
  //      limits | ncon × (normal, tangent, tangent)]. Lane r keeps its row's velocity
  //      w_r = J_r u, λ_r and constants; every lane forms its own row's candidate update
  //      and only the row being swept keeps it (a select), so a row costs one readlane of
  //      its Δλ, broadcast into w += A[·][r] Δλ. The tangent pair trades its two candidates
  //      between neighbouring lanes by DPP for the friction-disk norm. A contact's three
  //      A columns are loaded one contact ahead.
  {
    float w = w0, lam = 0.f;
    const float mu = s.mu;
    auto wave_shl1 = [](float v) {  // lane x receives lane x + 1 (wave-wide shift)
      return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x130, 0xf, 0xf, false));
    };
    auto wave_shr1 = [](float v) {  // lane x receives lane x - 1
      return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x138, 0xf, 0xf, false));
    };
    const float tg = row_lane ? s.tgt[lane] : 0.f;
    const float ia = row_lane ? 1.0f / s.Arr[lane] : 0.f;
    const int rlast = max(nrows - 3, 0);      // first row of the last contact
    const int lc = max(min(lane, nrows - 1), 0);  // lanes past the rows read a valid (unused) entry
    // A[r][lane]: square, from the packed triangle (row r up to the diagonal, then column r),
    // or formed on the fly (lanes past the rows have y = J_l = 0 and read 0)
    const int tl = lc * (lc + 1) / 2;
    auto arow_sq = [&](int r) { return Am[r * nrows + lc]; };
    auto arow_tri = [&](int r) { return Am[lc <= r ? r * (r + 1) / 2 + lc : tl + r]; };
    // either form per lane, without a branch: the triangle index of (max, min) (24-bit products)
    auto arow_mix = [&](int r) {
      const int hi = max(r, lc), lo = min(r, lc);
      const int it = (mul24(hi, hi + 1) >> 1) + lo;
      const int is = mul24(r, nrows) + lc;
      return Am[tri ? it : is];
    };
    // keep a or take b where m, as a bitwise select (no branch)
    auto sel = [](bool m, float a, float b) {
      const int k = -(int)m;
      return __int_as_float((__float_as_int(b) & k) | (__float_as_int(a) & ~k));
    };
    auto arow_otf = [&](int r) {
      const float* zg = ZG + r * RW;
      const float v = yr[0] * zg[0] + yr[1] * zg[1] + yr[2] * zg[2] + yr[3] * zg[3] + yr[4] * zg[4] + yr[5] * zg[5];
      const float vl = jlr[0] * zg[6] + jlr[1] * zg[7] + jlr[2] * zg[8];
      return v + (s.rleg[r] == lr ? vl : 0.f);
    };
    // the groups' row counts as wave-uniform scalars (the loops run to the larger; a group past
    // its own count changes nothing)
    const int NLm = gmax<WL>(nlim), NCm = gmax<WL>(ncon);
    const int nl0 = gval<WL>(nlim, 0), nl1 = WL == 64 ? nl0 : gval<WL>(nlim, 1);
    // the sweeps, instantiated for each form of A (the square one carries no index selects)
    auto sweeps = [&](auto arow) {
      for (int it = 0; it < Pm->solver_iterations; ++it) {
        for (int r = 0; r < NLm; ++r) {
          const bool on = WL == 64 || r < nlim;
          const float a0 = on ? arow(r) : 0.f;
          const float cand = fmaxf(0.f, lam + (tg - w) * ia);
          const float d = gbcast<WL>(cand - lam, min(r, 31), min(r, 31));
          lam = sel(lane == r && on, lam, cand);
          w += on ? a0 * d : 0.f;
        }
        if (NCm == 0) continue;
        float n0 = arow(min(nlim, rlast)), n1 = arow(min(nlim + 1, rlast + 1)), n2 = arow(min(nlim + 2, rlast + 2));
        for (int c = 0; c < NCm; ++c) {
          const bool on = WL == 64 || c < ncon;
          const int r = nlim + 3 * c;                               // this group's row
          const int ra = nl0 + 3 * c, rb = nl1 + 3 * c;             // each group's, uniform
          const int ra_ = WL == 64 ? ra : min(ra, WL - 3), rb_ = WL == 64 ? rb : min(rb, WL - 3);
          const float a0 = on ? n0 : 0.f, a1 = on ? n1 : 0.f, a2 = on ? n2 : 0.f;
          const int rn = min(r + 3, rlast);
          n0 = arow(rn);
          n1 = arow(rn + 1);
          n2 = arow(rn + 2);
          // normal row
          const float cand = fmaxf(0.f, lam + (tg - w) * ia);
          const float d = gbcast<WL>(cand - lam, ra_, rb_);
          lam = sel(lane == r && on, lam, cand);
          w += a0 * d;
          // tangent pair, projected onto the friction disk |λ_t| <= μ λ_n
          const float lim = mu * gbcast<WL>(lam, ra_, rb_);
          const float l = lam - w * ia;
          // both shifts with every lane active (a DPP source lane outside EXEC reads 0), then
          // the select: lane r + 1 takes r + 2's candidate, lane r + 2 takes r + 1's (the pair
          // never straddles the two groups: r + 2 < WL)
          float from_next = wave_shl1(l), from_prev = wave_shr1(l);
          __asm__ volatile("" : "+v"(from_next), "+v"(from_prev));
          const float other = lane == r + 1 ? from_next : from_prev;
          const float nn = l * l + other * other;
          const float sc = nn > lim * lim ? lim * __builtin_amdgcn_rsqf(nn) : 1.0f;
          const float lt = l * sc;
          const float dl = lt - lam;
          const float d1 = gbcast<WL>(dl, ra_ + 1, rb_ + 1), d2 = gbcast<WL>(dl, ra_ + 2, rb_ + 2);
          lam = sel((unsigned)(lane - r - 1) < 2u && on, lam, lt);
          w += a1 * d1 + a2 * d2;
        }
      }
    };
    if constexpr (WL == 64) {
      if (!stored) sweeps(arow_otf);
      else if (tri) sweeps(arow_tri);
      else sweeps(arow_sq);
    } else {
      sweeps(arow_mix);
    }
    if (row_lane) s.lam[lane] = lam;
  }
  __syncthreads();
  PH(8);
}

// one physics substep (legged_robot.py:80-85 loop body) of the group's env. WL = the env's lanes
// (see grp_of_lane); with two envs per wave, S0 / A0 / astride locate both envs' Sh and arenas
// for the wide constraint solve (an env with more than 32 rows: each env in turn on all 64 lanes).
template <bool TERRAIN, bool ACTNET, int WL, bool FORCE>
LGX_DEV void substep(Sh& s, float* A, Sh* S0, float* A0, int astride, const lgx_model* M_,
                     const lgx_task_params* Pm_, const lgx_buffers& B, int lane_, int e, int sub, bool last) {
  // The model and task tables are re-read each substep (L1 / scalar-cache hits) rather than
  // hoisted out of the decimation loop, where ~40 lane-indexed constants would otherwise stay
  // live in VGPRs across the whole step. Likewise the lane index, so that per-lane index and
  // LDS-address arithmetic is recomputed each substep instead of being hoisted and spilled.
  const lgx_model* M = opaque(M_);
  const lgx_task_params* Pm = opaque(Pm_);
  const int lane = opaque_lane(lane_);
  const float dt = Pm->sim_dt;
  // ---- PD torques: LeggedRobot._compute_torques legged_robot.py:440-478
  {
#pragma clang fp contract(off)
    if (ACTNET) {
      sea_torques_lanes(s, A, Pm, B, e, lane, sub);
    } else if (lane < NJ) {
      const int j = lane;
      float as = s.act[j] * Pm->action_scale;
      float t;
      if (Pm->control_type == LGX_CONTROL_P) {
        float err = (as + Pm->default_dof_pos[j]) - s.th[j];
        if (Pm->randomize_kp_kd)
          t = (s.kpm[j] * Pm->p_gains[j]) * err - (s.kdm[j] * Pm->d_gains[j]) * s.thd[j];
        else
          t = Pm->p_gains[j] * err - Pm->d_gains[j] * s.thd[j];
      } else if (Pm->control_type == LGX_CONTROL_V) {
        t = Pm->p_gains[j] * (as - s.thd[j]) - Pm->d_gains[j] * ((s.thd[j] - s.ldv[j]) / Pm->sim_dt);
      } else {
        t = as;
      }
      if (B.motor_strength) t = motor_strength(Pm, B, e, j) * t;
      s.tau[j] = fminf(fmaxf(t, -Pm->torque_limits[j]), Pm->torque_limits[j]);
    }
  }
  PH(1);
  kinematics<true, FORCE>(s, A, M, Pm, lane);
  PH(2);
  DynOut dy;
  dynamics(s, A, lane, dy);
  const int jl_ = lane < NJ ? lane : NJ - 1, leg_ = jl_ / 3, pos_ = jl_ % 3;  // joint lanes' leg / chain position
  // ---- free velocity u* = u + dt M⁻¹ f, f = [−h_B ; τ − h_J] (factored form, see dynamics)
  const float fj = lane < NJ ? s.tau[lane] - dy.hj : 0.f;
  if (lane < NJ) s.up[lane] = fj;  // scratch: f_J, read by the leg's lanes below
  float vb[6];
#pragma unroll
  for (int r = 0; r < 6; ++r) vb[r] = -dy.hb[r] - grow_sum16<WL>(dy.xj[r] * fj);
  __syncthreads();  // S⁻¹ (dynamics) and f_J visible
  PH(3);
  {
    float zb[6];
#pragma unroll
    for (int r = 0; r < 6; ++r) {
      const float* Si = s.Sinv[r];
      zb[r] = Si[0] * vb[0] + Si[1] * vb[1] + Si[2] * vb[2] + Si[3] * vb[3] + Si[4] * vb[4] + Si[5] * vb[5];
    }
    if (lane < 6) {
      const float* Si = s.Sinv[lane];
      const float zl = Si[0] * vb[0] + Si[1] * vb[1] + Si[2] * vb[2] + Si[3] * vb[3] + Si[4] * vb[4] + Si[5] * vb[5];
      const float u0 = lane < 3 ? s.vo[lane] : s.wb[lane - 3];
      s.us[lane] = u0 + dt * zl;
    }
    if (lane < NJ) {
      const float* fl = s.up + 3 * leg_;
      float bot = dy.dinv[0] * fl[0] + dy.dinv[1] * fl[1] + dy.dinv[2] * fl[2];
#pragma unroll
      for (int r = 0; r < 6; ++r) bot -= dy.xj[r] * zb[r];
      s.us[6 + lane] = s.thd[lane] + dt * bot;
    }
  }
  PH(4);
  // ---- constraint detection: joint limits (lanes 0..11), contacts (one candidate per lane, in
  //      rounds of WL candidates: the rows keep the candidates' order)
  bool lim_lo = false, lim_hi = false;
  if (lane < NJ && M->joint_has_limits[lane + 1]) {
    lim_lo = s.th[lane] < M->joint_lower[lane + 1] + Pm->limit_margin;
    lim_hi = !lim_lo && s.th[lane] > M->joint_upper[lane + 1] - Pm->limit_margin;
  }
  const uint64_t lmask = gballot<WL>(lim_lo || lim_hi);
  const int nlim = __popcll(lmask);
  const uint64_t below = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
  auto target = [&](float d) {
    float tv;
    if (d > Pm->slop) tv = fminf(Pm->baumgarte * (d - Pm->slop) / dt, Pm->max_depenetration_vel);
    else if (d >= 0.f) tv = 0.f;
    else tv = d / dt;
    return tv;
  };
  float* const J9 = A + MAXR * RW;    // [nrows][RW]: J_B (6) | J of leg rleg (3)
  constexpr bool plane = !TERRAIN;  // the launch picks the variant from mesh_type
  // every candidate's contact query first (the trimesh query uses the arena the rows go to),
  // then the rows: limits, then contacts in candidate order
  constexpr int CR = (LGX_MAX_CANDIDATES + WL - 1) / WL;
  bool act[CR];
  f3 xc[CR], nrm[CR];
  float depth[CR];
  int ck[CR];
#pragma unroll
  for (int cr = 0; cr < CR; ++cr) {
    act[cr] = false;
    xc[cr] = mk(0, 0, 0);
    nrm[cr] = mk(0.f, 0.f, 1.f);
    depth[cr] = 0.f;
    ck[cr] = 0;
    if (cr * WL >= M->num_candidates) continue;  // uniform
    const int ci = cr * WL + lane;
    const bool cand = ci < M->num_candidates;
    if constexpr (plane) {
      if (cand) {
        ck[cr] = M->cand_link[ci];
        xc[cr] = ld3(s.P[ck[cr]]) + mv(s.R[ck[cr]], ld3(M->cand_pos[ci]));
        const float r = M->cand_radius[ci];
        depth[cr] = r - xc[cr].z;
        xc[cr].z -= r;
        act[cr] = depth[cr] > -Pm->contact_margin;
      }
    } else {
      float r = 0.f;
      if (cand) {
        ck[cr] = M->cand_link[ci];
        xc[cr] = ld3(s.P[ck[cr]]) + mv(s.R[ck[cr]], ld3(M->cand_pos[ci]));
        r = M->cand_radius[ci];
      }
      const TerrainHit th = terrain_contact_wave<WL>(Pm, B, A, xc[cr], r, cand, lane);
      if (cand) {
        depth[cr] = th.depth;
        nrm[cr] = th.n;
        xc[cr] = xc[cr] - nrm[cr] * r;  // deepest sphere point
        act[cr] = depth[cr] > -Pm->contact_margin;
      }
    }
  }
  if (lim_lo || lim_hi) {
    const int r = __popcll(lmask & below);
    float* jr = J9 + r * RW;
#pragma unroll
    for (int q = 0; q < RW; ++q) jr[q] = 0.f;
    jr[6 + pos_] = lim_lo ? 1.f : -1.f;
    const float d = lim_lo ? (M->joint_lower[lane + 1] - s.th[lane]) : (s.th[lane] - M->joint_upper[lane + 1]);
    s.tgt[r] = target(d);
    s.rleg[r] = leg_;
  }
  int nfound = 0;  // contacts of the earlier rounds (group-uniform)
#pragma unroll
  for (int cr = 0; cr < CR; ++cr) {
    if (cr * WL >= M->num_candidates) continue;  // uniform
    const int ci = cr * WL + lane;
    const uint64_t cmask = gballot<WL>(act[cr]);
    const int crank = nfound + __popcll(cmask & below);
    nfound += __popcll(cmask);
    if (act[cr] && crank < MAXC) {
      const int r0 = nlim + 3 * crank;
      const f3 p0 = ld3(s.P[0]);
      f3 dn = mk(0, 0, 1), dt1 = mk(1, 0, 0), dt2 = mk(0, 1, 0);
      if constexpr (!plane) {
        dn = nrm[cr];
        contact_tangents(nrm[cr], dt1, dt2);
      }
      st3(s.cn[crank], dn);
      const int leg = ck[cr] > 0 ? (ck[cr] - 1) / 3 : -1;
      const int pos = ck[cr] > 0 ? (ck[cr] - 1) % 3 : -1;
      const int kl = ck[cr] > 0 ? 1 + 3 * leg : 1;
      const f3 ax0 = ld3(s.Ax[kl]), ax1 = ld3(s.Ax[kl + 1]), ax2 = ld3(s.Ax[kl + 2]);
      const f3 r0p = xc[cr] - ld3(s.P[kl]), r1p = xc[cr] - ld3(s.P[kl + 1]), r2p = xc[cr] - ld3(s.P[kl + 2]);
      const f3 rb = xc[cr] - p0;
#pragma unroll
      for (int t = 0; t < 3; ++t) {
        const int r = r0 + t;
        const f3 d = t == 0 ? dn : (t == 1 ? dt1 : dt2);
        const f3 ang = cross(rb, d);
        float* jr = J9 + r * RW;
        jr[0] = d.x; jr[1] = d.y; jr[2] = d.z;
        jr[3] = ang.x; jr[4] = ang.y; jr[5] = ang.z;
        jr[6] = pos >= 0 ? dot(ax0, cross(r0p, d)) : 0.f;
        jr[7] = pos >= 1 ? dot(ax1, cross(r1p, d)) : 0.f;
        jr[8] = pos >= 2 ? dot(ax2, cross(r2p, d)) : 0.f;
        s.rleg[r] = leg;
        s.tgt[r] = t == 0 ? target(depth[cr]) : 0.f;
      }
      s.cbody[crank] = M->cand_body[ci];
    }
  }
  const int ncon = min(nfound, MAXC);
  const int nrows = nlim + 3 * ncon;
  const int nrw = gmax<WL>(nrows);  // the wave's largest system
#if LGX_ROW_PRIO > 0
  // Issue priority by constraint-system size (s_setprio 0..3 above 0 / t / 2t / 3t rows): a
  // launch lasts as long as its slowest wave, and the waves with the largest systems are the
  // slow ones; the SIMD's other waves have the slack (profiles/r03_wave_priority.txt).
  {
    const int rp = nrw > LGX_ROW_PRIO * 3 ? 3 : nrw > LGX_ROW_PRIO * 2 ? 2 : nrw > LGX_ROW_PRIO ? 1 : 0;
    set_prio(LGX_SLOT_PRIO ? max(rp, min(wave_slot(), 3)) : rp);
  }
#endif
  if (lane == 0) { s.nrows = nrows; s.nlim = nlim; s.ncon = ncon; }
#ifdef LGX_PHASE_CLOCK
  if (lane == 0) {
    s.phacc[16] = max(s.phacc[16], (uint32_t)nrows);
    s.phacc[17] += nrows > AMAX ? 1u : 0u;
  }
#endif
  __syncthreads();
  PH(5);
  if constexpr (WL == 64) {
    solve_rows<64>(s, A, Pm, lane, nrows, nlim, ncon);
  } else if (nrw <= WL) {
    solve_rows<WL>(s, A, Pm, lane, nrows, nlim, ncon);
  } else {
    // an env of this wave has more rows than its group has lanes (a fallen robot): each env's
    // solve in turn on the whole wave (its rows from LDS; the same numbers)
    const int wl = (int)__lane_id();
#pragma unroll 1
    for (int g = 0; g < 64 / WL; ++g) {
      Sh& sg = S0[g];
      const int nr = gval<WL>(nrows, g), nli = gval<WL>(nlim, g), nco = gval<WL>(ncon, g);
      solve_rows<64>(sg, A0 + (size_t)g * astride, Pm, wl, nr, nli, nco);
    }
  }
  // ---- u+ = u* + M⁻¹ Jᵀ λ = u* + [Z ; G_J − Xᵀ Z]:  Z = Σ_r λ_r z_r,
  //      G_j = Σ_{r on leg(j)} λ_r g_r[pos(j)]
  {
    const float* const ZG = A;
    float Z[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f}, G = 0.f;
#pragma unroll 4
    for (int r = 0; r < nrw; ++r) {
      if (WL == 64 || r < nrows) {
        const float lr_ = s.lam[r];
        const float* zg = ZG + r * RW;
#pragma unroll
        for (int q = 0; q < 6; ++q) Z[q] += lr_ * zg[q];
        const float gq = pos_ == 0 ? zg[6] : (pos_ == 1 ? zg[7] : zg[8]);
        G += s.rleg[r] == leg_ ? lr_ * gq : 0.f;
      }
    }
    if (lane < 6) {
      float zl = 0.f;
#pragma unroll
      for (int q = 0; q < 6; ++q) zl = lane == q ? Z[q] : zl;
      s.up[lane] = s.us[lane] + zl;
    }
    if (lane < NJ) {
      const float* Xj = s.X[lane];
      float v = s.us[6 + lane] + G;
#pragma unroll
      for (int q = 0; q < 6; ++q) v -= Xj[q] * Z[q];
      s.up[6 + lane] = v;
    }
  }
  __syncthreads();
  PH(9);
  // ---- contact forces of the last substep, per reported body (world frame)
  if (last && lane < LGX_MAX_BODIES) {
    float f[3] = {0.f, 0.f, 0.f};
    const int ncm = gmax<WL>(ncon);
    for (int c = 0; c < ncm; ++c) {
      if (c >= ncon || s.cbody[c] != lane) continue;
      const int r = nlim + 3 * c;
      if constexpr (!TERRAIN) {
        f[2] += s.lam[r]; f[0] += s.lam[r + 1]; f[1] += s.lam[r + 2];
      } else {
        f3 t1, t2;
        const f3 n = ld3(s.cn[c]);
        contact_tangents(n, t1, t2);
        const f3 fc = n * s.lam[r] + t1 * s.lam[r + 1] + t2 * s.lam[r + 2];
        f[0] += fc.x; f[1] += fc.y; f[2] += fc.z;
      }
    }
    s.cf[lane][0] = f[0] / dt; s.cf[lane][1] = f[1] / dt; s.cf[lane][2] = f[2] / dt;
  }
  // ---- semi-implicit Euler
  if (lane == 0) {
    f3 v = mk(s.up[0], s.up[1], s.up[2]), w = mk(s.up[3], s.up[4], s.up[5]);
#pragma unroll
    for (int i = 0; i < 3; ++i) s.pb[i] += dt * s.up[i];
    float wn = sqrtf(dot(w, w));
    float ang = wn * dt;
    float dq[4];
    if (ang > 1e-12f) {
      float sc = sinf(0.5f * ang) / wn;
      dq[0] = w.x * sc; dq[1] = w.y * sc; dq[2] = w.z * sc; dq[3] = cosf(0.5f * ang);
    } else {
      dq[0] = 0.5f * dt * w.x; dq[1] = 0.5f * dt * w.y; dq[2] = 0.5f * dt * w.z; dq[3] = 1.f;
    }
    const float* q = s.qb;
    float qn[4];
    qn[3] = dq[3] * q[3] - (dq[0] * q[0] + dq[1] * q[1] + dq[2] * q[2]);
    qn[0] = dq[3] * q[0] + q[3] * dq[0] + (dq[1] * q[2] - dq[2] * q[1]);
    qn[1] = dq[3] * q[1] + q[3] * dq[1] + (dq[2] * q[0] - dq[0] * q[2]);
    qn[2] = dq[3] * q[2] + q[3] * dq[2] + (dq[0] * q[1] - dq[1] * q[0]);
    float nq = rsqrtf(qn[0] * qn[0] + qn[1] * qn[1] + qn[2] * qn[2] + qn[3] * qn[3]);
#pragma unroll
    for (int i = 0; i < 4; ++i) s.qb[i] = qn[i] * nq;
    st3(s.vo, v);
    st3(s.wb, w);
  }
  if (lane < NJ) {
    s.thd[lane] = s.up[6 + lane];
    s.th[lane] += dt * s.thd[lane];
  }
  __syncthreads();
  PH(10);
}

#pragma clang fp contract(off)

// ============================================================== post-physics helpers
// (fp32, no contraction: the reference evaluates these as separate eager torch ops)

// reset_idx for one env (go2.py:207-263 / legged_robot.py:157-213). The env's root/dof/
// command state is in LDS (s.root, s.th, s.thd, s.cmd, s.ep): lane 0 does the scalar part,
// lanes write the per-env buffer rows. Called under a uniform branch.
template <int WL>
LGX_DEV void reset_env(const lgx_task_params* Pm, const lgx_buffers& B, Sh& s, float* A, int e, int lane,
                       bool after_init, bool zero_carried, bool sums_in_lds) {
  const int D = Pm->num_dof;
  const float* U = stg_U(A);
  if (lane == 0) reset_env_head(Pm, B, s, U, e, after_init);
  // _reset_dofs legged_robot.py:481-506: q = q0 + U(0, 0.9), qd = 0
  if (lane < D) {
    s.th[lane] = Pm->default_dof_pos[lane] + rand_range(0.0f, 0.9f, U[S_DOF + lane]);
    s.thd[lane] = 0.0f;
  }
  // buffer zeroing. Inside a step the last_* buffers and the history are rewritten at the
  // end of post_physics_step anyway (go2.py:380-384, 570-574); only an external reset
  // has to zero them.
  if (zero_carried) {
    const int A = Pm->num_actions, H = Pm->history_len * Pm->num_proprio;
    if (lane < A) B.last_actions[(size_t)e * A + lane] = 0.f;
    if (B.action_history)
      for (int i = lane; i < Pm->action_history_len * A; i += WL) B.action_history[(size_t)e * Pm->action_history_len * A + i] = 0.f;
    if (lane < D) { B.last_dof_vel[(size_t)e * D + lane] = 0.f; B.last_torques[(size_t)e * D + lane] = 0.f; }
    if (lane < 6) B.last_root_vel[e * 6 + lane] = 0.f;
    if (lane < 3) B.last_base_lin_vel[e * 3 + lane] = 0.f;
    for (int i = lane; i < H; i += WL) B.obs_history[(size_t)e * H + i] = 0.f;
  }
  if (Pm->actuator_net && lane < 2 * D) {  // Anymal.reset_idx anymal.py:56-60: zero h, c
    const size_t NT = (size_t)Pm->num_envs * D;
    const int l = lane / D, j = lane % D;
    float4* hp = reinterpret_cast<float4*>(B.sea_hidden + (l * NT + (size_t)e * D + j) * 8);
    float4* cp = reinterpret_cast<float4*>(B.sea_cell + (l * NT + (size_t)e * D + j) * 8);
    hp[0] = hp[1] = cp[0] = cp[1] = make_float4(0.f, 0.f, 0.f, 0.f);
  }
  if (Pm->task_kind == LGX_TASK_GO2 && lane < Pm->num_feet) {
    if (B.feet_air_time) B.feet_air_time[e * Pm->num_feet + lane] = 0.f;
    B.last_contacts[e * Pm->num_feet + lane] = 0;
    B.last_contact_heights[e * Pm->num_feet + lane] = 0.f;
  }
  const int K = Pm->num_reward_terms + (Pm->has_termination_reward ? 1 : 0);
  for (int k = lane; k < K; k += WL) {
    float* es = B.episode_sums + (size_t)e * K + k;
    const float sum = sums_in_lds ? s.es[k] : *es;  // in a step: this step's updated row, staged in LDS
    if (B.episode_stats) atomicAdd(B.episode_stats + k, sum);
    // the command curriculum's input (go2.py:87): this env's tracking_lin_vel sum at its reset
    if (sums_in_lds && B.curriculum_vals && k == Pm->curriculum_term) B.curriculum_vals[e] = sum;
    *es = 0.f;
  }
  if (lane == 0 && B.episode_stats) atomicAdd(B.episode_stats + K, 1.0f);
  __syncthreads();
}

template <int WL>
LGX_DEV void fill_uniforms(float* A, uint64_t seed, uint32_t gid, uint64_t step, uint32_t stream, int lane, int nblk) {
  for (int b = lane; b < nblk; b += WL) {
    uint32_t o[4];
    philox4x32_10(gid, (uint32_t)step, (uint32_t)b | (stream << 16), (uint32_t)(step >> 32), (uint32_t)seed,
                  (uint32_t)(seed >> 32), o);
    float* U = stg_U(A);
    U[4 * b + 0] = u01(o[0]); U[4 * b + 1] = u01(o[1]);
    U[4 * b + 2] = u01(o[2]); U[4 * b + 3] = u01(o[3]);
  }
  __syncthreads();
}

// The sums over joints (and height points) that reward terms use, formed lane-parallel
// (lane j = joint j, reduced over lanes 0..15 by a DPP scan; lane 15 writes them), so the
// per-term lanes below do no joint loops. Summation order differs from torch's sum over a
// dim by ~1 ulp of the sum (golden tests: 1e-5).
LGX_DEV void joint_sums(const lgx_task_params* Pm, const lgx_buffers& B, Sh& s, float* A, int e, int lane) {
  const int D = Pm->num_dof;
  const int j = lane < D ? lane : 0;
  const float on = lane < D ? 1.0f : 0.0f;
  const float la = s.la_prev[j], lt = s.lt_prev[j];  // prefetched at kernel start
  const float q = s.th[j], qd = s.thd[j], tau = s.tau[j], q0 = Pm->default_dof_pos[j];
  const float dq = q - q0;
  float v[J_N];
  v[J_ACTION_RATE] = sq(la - s.act[j]);
  v[J_DELTA_TORQUES] = sq(tau - lt);
  v[J_DOF_ACC] = sq((s.ldv[j] - qd) / Pm->dt);
  v[J_DOF_ERROR] = sq(dq);
  {
    const float lo = q - Pm->dof_pos_limits[j][0], hi = q - Pm->dof_pos_limits[j][1];
    float o = -(lo < 0.0f ? lo : 0.0f);
    o += (hi > 0.0f ? hi : 0.0f);
    v[J_DOF_POS_LIMITS] = o;
  }
  v[J_DOF_VEL] = sq(qd);
  v[J_DOF_VEL_LIMITS] = clipf(fabsf(qd) - Pm->dof_vel_limits[j] * Pm->soft_dof_vel_limit, 0.0f, 1.0f);
  v[J_STAND_ABS] = fabsf(dq);
  {
    const float t = fabsf(tau) - Pm->torque_limits[j] * Pm->soft_torque_limit;
    v[J_TORQUE_LIMITS] = t > 0.0f ? t : 0.0f;
  }
  v[J_TORQUES] = sq(tau);
  float hip = 0.f, thigh = 0.f, calf = 0.f;
  for (int i = 0; i < 4; ++i) {
    hip += Pm->hip_joint_idx[i] == j ? 1.f : 0.f;
    thigh += Pm->thigh_joint_idx[i] == j ? 1.f : 0.f;
    calf += Pm->calf_joint_idx[i] == j ? 1.f : 0.f;
  }
  v[J_HIP_POS] = hip * v[J_DOF_ERROR];
  v[J_THIGH_POS] = thigh * v[J_DOF_ERROR];
  v[J_CALF_POS] = calf * v[J_DOF_ERROR];
  // height points: lane i < 16 sums points i, i + 16, ...
  float hsum = 0.f;
  if (lane < 16) {
    const float* hts = stg_heights(A, Pm);
    for (int i = lane; i < Pm->num_height_points; i += 16) hsum += s.root[2] - hts[i];
  }
#pragma unroll
  for (int k = 0; k < J_N; ++k) {
    float x = k == J_HEIGHT ? (lane < 16 ? hsum : 0.f) : v[k] * on;
    x += dpp_shr_t<0x111>(x);
    x += dpp_shr_t<0x112>(x);
    x += dpp_shr_t<0x114>(x);
    x += dpp_shr_t<0x118>(x);
    if (lane == 15) s.jsum[k] = x;
  }
}

template <int WL>
LGX_DEV void get_heights(const lgx_task_params* Pm, const lgx_buffers& B, Sh& s, float* A, int lane) {
  const int NP = Pm->num_height_points;
  const float* root = s.root;
  if (Pm->mesh_type == LGX_MESH_PLANE || B.height_samples == nullptr) {
    for (int i = lane; i < NP; i += WL) stg_heights(A, Pm)[i] = 0.0f;
    return;
  }
  float qy[4];
  scan_yaw_quat(root[5], root[6], qy);
  for (int i = lane; i < NP; i += WL)
    stg_heights(A, Pm)[i] = scan_point_height(Pm, B.height_samples, qy, root, Pm->height_points[i][0],
                                              Pm->height_points[i][1]);
}

// ============================================================== kernels
// Occupancy target: 4 waves per SIMD (<= 128 VGPRs; the Go2 LDS image is 9.6 KB, so 4096
// envs are one residency round on 256 CUs). The SEA-LSTM variant keeps its hidden states in
// registers (fewer waves per SIMD; ANYmal's LDS image is 13 KB).
#ifndef LGX_SEA_WAVES
#define LGX_SEA_WAVES 4
#endif
// EPW envs per wave (1, or 2: each env on a 32-lane group, grp_of_lane; blocks = N / 2, envs 2b'
// and 2b' + 1 of the XCD-aware pair order b' = env_of_block). Each env has its own Sh and LDS arena.
// Two envs per wave: LDS holds 2 x (Sh + arena) per block, so 8 blocks per CU (2 waves per
// SIMD) are resident — the register budget is that of 2 waves per SIMD.
// SENSOR: the instances with the sensor model (include/lgx.h, ABI 15), launched when one of its
// buffers is bound; the others hold none of its code.
// FORCE: likewise the instances with the external force (include/lgx.h, ABI 16), launched when its
// buffers are bound.
template <bool PHYSICS, bool TERRAIN, bool ACTNET, int EPW, bool SENSOR, bool FORCE>
__global__ __launch_bounds__(64, ACTNET ? LGX_SEA_WAVES : (EPW == 2 ? 2 : 4)) void env_step_kernel(const lgx_model* __restrict__ M,
                                                      const lgx_task_params* __restrict__ Pm,
                                                      const lgx_buffers* __restrict__ Bp, uint64_t seed,
                                                      uint64_t step_arg, const uint64_t* __restrict__ step_dev) {
  constexpr int WL = 64 / EPW;  // lanes per env
  __shared__ Sh S_[EPW];
  const int grp = grp_of_lane<WL>();
  Sh& s = S_[grp];
  const int astride = (int)arena_floats(*Pm);
  float* const AR = lgx_dyn + (EPW == 1 ? 0 : grp * astride);  // this env's arena
  // buffer pointers are read from device memory (scalar loads) when used, not held in SGPRs
  const lgx_buffers& B = *Bp;
  // graph-replayable form: the step counter is read from device memory (lgx_step_dev)
  const uint64_t step = step_dev ? *step_dev : step_arg;
  const int e = EPW * env_of_block(blockIdx.x, gridDim.x) + grp;
  const int lane = EPW == 1 ? (int)threadIdx.x : (int)(threadIdx.x & (WL - 1));
#if LGX_SLOT_PRIO
  // the SIMD's arbiter favours its older waves; a launch ends with its slowest wave, so the
  // younger slots get the higher issue priority
  set_prio(min(wave_slot(), 3));
#endif
  const int D = Pm->num_dof, A = Pm->num_actions, NB = Pm->num_bodies;
  const uint32_t gid = (uint32_t)(Pm->env_id_offset + e);

  // ---------------------------------------------------------------- load + clip
  float* root_g = B.root_states + (size_t)e * 13;
  if (lane < A) {
    float a = B.actions_in[(size_t)e * A + lane];
    a = clipf(a, -Pm->clip_actions, Pm->clip_actions);  // legged_robot.py:74-75
    s.act[lane] = a;
    B.actions[(size_t)e * A + lane] = a;
  }
  if (lane < D) {
    s.th[lane] = B.dof_state[((size_t)e * D + lane) * 2];
    s.thd[lane] = B.dof_state[((size_t)e * D + lane) * 2 + 1];
    s.kpm[lane] = B.kp_kd ? B.kp_kd[(size_t)e * D + lane] : 1.f;
    s.kdm[lane] = B.kp_kd ? B.kp_kd[((size_t)Pm->num_envs + e) * D + lane] : 1.f;
    s.ldv[lane] = B.last_dof_vel[(size_t)e * D + lane];
  }
  if (lane < 13) s.root[lane] = root_g[lane];
  if (lane == 0) {
    s.madd = B.mass_params ? B.mass_params[e * 4] : 0.f;
    s.mu = 0.5f * ((B.friction ? B.friction[e] : 1.f) + Pm->ground_friction);
  }
  if (lane < 3) s.cadd[lane] = B.mass_params ? B.mass_params[e * 4 + 1 + lane] : 0.f;
  if (lane < 4) s.cmd[lane] = B.commands[e * 4 + lane];
  if (lane == 0) {
    s.blew = 0;
    s.ep_prev = B.episode_length[e];
    s.jump_prev = B.rpy_phase ? B.rpy_phase[e * 8 + 7] : 0.f;
    s.fric = B.friction ? B.friction[e] : 1.f;
  }
  // inputs the post-physics phase reads (their latency hides behind the physics)
  if (lane < A) s.la_prev[lane] = B.last_actions[(size_t)e * A + lane];
  if (lane < D) s.lt_prev[lane] = B.last_torques[(size_t)e * D + lane];
  {
    const int KS0 = Pm->num_reward_terms + (Pm->has_termination_reward ? 1 : 0);
    for (int k = lane; k < KS0; k += WL) s.es[k] = B.episode_sums[(size_t)e * KS0 + k];
  }
  if (Pm->task_kind == LGX_TASK_GO2 && lane < Pm->num_feet) {
    s.lc_prev[lane] = B.last_contacts[e * Pm->num_feet + lane];
    s.lch_prev[lane] = B.last_contact_heights[e * Pm->num_feet + lane];
    s.fat_prev[lane] = B.feet_air_time ? B.feet_air_time[e * Pm->num_feet + lane] : 0.f;
  }
#ifdef LGX_PHASE_CLOCK
  if (lane < 20) s.phacc[lane] = 0u;
  if (lane == 0) s.phlast = clock64();
#endif
  __syncthreads();

  if (PHYSICS) {
    if (lane == 0) {
      float q[4] = {s.root[3], s.root[4], s.root[5], s.root[6]};
      float n = rsqrtf(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
      for (int i = 0; i < 4; ++i) s.qb[i] = q[i] * n;
      for (int i = 0; i < 3; ++i) { s.pb[i] = s.root[i]; s.wb[i] = s.root[10 + i]; }
      float R[9];
      quat_to_R(s.qb, R);
      f3 rc = mv(R, mk(M->link_com[0][0] + s.cadd[0], M->link_com[0][1] + s.cadd[1], M->link_com[0][2] + s.cadd[2]));
      f3 vo = ld3(s.root + 7) - cross(ld3(s.wb), rc);  // COM velocity -> origin velocity
      st3(s.vo, vo);
      // external force (include/lgx.h, ABI 16): the window at the episode length this step will
      // write, the world vector from the quaternion the step starts from; the substeps read LDS only
      if constexpr (FORCE) {
        s.rterm[FRC_ON] = 0.f;
        if (B.force_window) {
          const int32_t* fwin = B.force_window + (size_t)e * 3;
          const float* fv = B.force_vec + (size_t)e * 6;
          if (force_window_on(fwin[0], fwin[1], fwin[2], s.ep_prev + 1) && (fv[0] != 0.f || fv[1] != 0.f || fv[2] != 0.f)) {
            s.rterm[FRC_ON] = 1.f;
            force_to_world(s.root + 3, fv, s.rterm + FRC_F);
            for (int i = 0; i < 3; ++i) s.rterm[FRC_PT + i] = fv[3 + i];
          }
        }
      }
    }
    __syncthreads();
    PH(0);
    for (int sub = 0; sub < Pm->decimation; ++sub) {
      if (!ACTNET && B.action_delay) {  // (the actuator net: sea_action)
        stage_actuator_action(s, Pm, B, e, lane, sub);
        __syncthreads();
      }
      substep<TERRAIN, ACTNET, WL, FORCE>(s, AR, S_, lgx_dyn, astride, M, Pm, B, lane, e, sub, sub == Pm->decimation - 1);
    }
    // the rest of the step (guard, observation, last_actions, rewards) sees this step's action
    if (!ACTNET && B.action_delay) {
      const int ln = opaque_lane(lane), A = opaque(Pm)->num_actions;
      if (ln < A) s.act[ln] = B.actions[(size_t)e * A + ln];
    }
    __syncthreads();
    // NaN/Inf guard (SURVEY.md §5 "Failure detection"; the reference has none): a state that
    // went non-finite in any substep stays non-finite, so one check after the substeps sees it.
    // Such an env gets a finite stand-in state (default joint pose at its start position, at
    // rest, no torques / contact forces / actions), is flagged in blew_up, counted, and reset
    // below by the normal masked path, so no NaN reaches its observations, rewards or the
    // learner. Other envs are untouched.
    {
      bool bad = false;
      if (lane < D) bad = !(isfinite(s.th[lane]) && isfinite(s.thd[lane]) && isfinite(s.tau[lane]));
      if (lane < A) bad = bad || !isfinite(s.act[lane]);
      if (lane < 3) bad = bad || !(isfinite(s.pb[lane]) && isfinite(s.vo[lane]) && isfinite(s.wb[lane]));
      if (lane < 4) bad = bad || !isfinite(s.qb[lane]);
      if (lane < NB) bad = bad || !(isfinite(s.cf[lane][0]) && isfinite(s.cf[lane][1]) && isfinite(s.cf[lane][2]));
      if (gballot<WL>(bad) != 0ull) {
        if (lane < D) { s.th[lane] = Pm->default_dof_pos[lane]; s.thd[lane] = 0.f; s.tau[lane] = 0.f; }
        if (lane < A) { s.act[lane] = 0.f; B.actions[(size_t)e * A + lane] = 0.f; }
        if (lane < 3) { s.pb[lane] = isfinite(s.root[lane]) ? s.root[lane] : 0.f; s.vo[lane] = 0.f; s.wb[lane] = 0.f; }
        if (lane < 4) s.qb[lane] = lane == 3 ? 1.f : 0.f;
        if (lane < NB) { s.cf[lane][0] = 0.f; s.cf[lane][1] = 0.f; s.cf[lane][2] = 0.f; }
        if (lane == 0) {
          s.blew = 1;
          if (B.blowup_count) atomicAdd(B.blowup_count, 1u);
        }
      }
      __syncthreads();
    }
    // final kinematics for the rigid-body state tensor
    kinematics<false>(s, AR, M, Pm, lane);
    float root[13];
    {
      float R[9];
      quat_to_R(s.qb, R);
      f3 rc = mv(R, mk(M->link_com[0][0] + s.cadd[0], M->link_com[0][1] + s.cadd[1], M->link_com[0][2] + s.cadd[2]));
      f3 vc = ld3(s.vo) + cross(ld3(s.wb), rc);
      root[0] = s.pb[0]; root[1] = s.pb[1]; root[2] = s.pb[2];
      root[3] = s.qb[0]; root[4] = s.qb[1]; root[5] = s.qb[2]; root[6] = s.qb[3];
      root[7] = vc.x; root[8] = vc.y; root[9] = vc.z;
      root[10] = s.wb[0]; root[11] = s.wb[1]; root[12] = s.wb[2];
    }
    __syncthreads();
    if (lane < 13) s.root[lane] = root[lane];
    // rigid body states, contact forces, torques -> HBM
    if (lane < NB) {
      const int k = M->body_link[lane];
      f3 off = ld3(M->body_offset[lane]);
      f3 o = mv(s.R[k], off);
      f3 pos = ld3(s.P[k]) + o;
      bool primary = off.x == 0.f && off.y == 0.f && off.z == 0.f;
      f3 lv = ld3(s.V[k]) + cross(ld3(s.W[k]), primary ? (ld3(s.C[k]) - ld3(s.P[k])) : o);
      float Rb[9];
      mm(s.R[k], M->body_rot[lane], Rb);
      float tr = Rb[0] + Rb[4] + Rb[8], qq[4];
      if (tr > 0.f) {
        float sc = sqrtf(tr + 1.f) * 2.f;
        qq[3] = 0.25f * sc; qq[0] = (Rb[7] - Rb[5]) / sc; qq[1] = (Rb[2] - Rb[6]) / sc; qq[2] = (Rb[3] - Rb[1]) / sc;
      } else if (Rb[0] > Rb[4] && Rb[0] > Rb[8]) {
        float sc = sqrtf(1.f + Rb[0] - Rb[4] - Rb[8]) * 2.f;
        qq[3] = (Rb[7] - Rb[5]) / sc; qq[0] = 0.25f * sc; qq[1] = (Rb[1] + Rb[3]) / sc; qq[2] = (Rb[2] + Rb[6]) / sc;
      } else if (Rb[4] > Rb[8]) {
        float sc = sqrtf(1.f + Rb[4] - Rb[0] - Rb[8]) * 2.f;
        qq[3] = (Rb[2] - Rb[6]) / sc; qq[0] = (Rb[1] + Rb[3]) / sc; qq[1] = 0.25f * sc; qq[2] = (Rb[5] + Rb[7]) / sc;
      } else {
        float sc = sqrtf(1.f + Rb[8] - Rb[0] - Rb[4]) * 2.f;
        qq[3] = (Rb[3] - Rb[1]) / sc; qq[0] = (Rb[2] + Rb[6]) / sc; qq[1] = (Rb[5] + Rb[7]) / sc; qq[2] = 0.25f * sc;
      }
      if (qq[3] < 0.f) for (int i = 0; i < 4; ++i) qq[i] = -qq[i];
      float* rb = B.rigid_body_states + ((size_t)e * NB + lane) * 13;
      rb[0] = pos.x; rb[1] = pos.y; rb[2] = pos.z;
      rb[3] = qq[0]; rb[4] = qq[1]; rb[5] = qq[2]; rb[6] = qq[3];
      rb[7] = lv.x; rb[8] = lv.y; rb[9] = lv.z;
      const float* w = s.W[k];
      rb[10] = w[0]; rb[11] = w[1]; rb[12] = w[2];
      s.rbz[lane] = pos.z;
      float* cfo = B.contact_forces + ((size_t)e * NB + lane) * 3;
      cfo[0] = s.cf[lane][0]; cfo[1] = s.cf[lane][1]; cfo[2] = s.cf[lane][2];
    }
    if (lane < D) B.torques[(size_t)e * D + lane] = s.tau[lane];
    __syncthreads();
    PH(11);
  } else {
    // post-physics only: physics state supplied by the caller
    if (lane < NB) {
      const float* cfi = B.contact_forces + ((size_t)e * NB + lane) * 3;
      s.cf[lane][0] = cfi[0]; s.cf[lane][1] = cfi[1]; s.cf[lane][2] = cfi[2];
      s.rbz[lane] = B.rigid_body_states[((size_t)e * NB + lane) * 13 + 2];
    }
    if (lane < D) s.tau[lane] = B.torques[(size_t)e * D + lane];
    __syncthreads();
  }

  // ================================================================ post-physics
  // Go2Robot.post_physics_step go2.py:345-387 / LeggedRobot legged_robot.py:103-138.
  // Per-env scalars: lane 0, into LDS. Vectors: lane-parallel from LDS.
  // the old observation history (read back at the end of the step) in flight from here on:
  // the first HV x 64 entries into registers (all of Go2's 5 x 52)
  constexpr int HV = 320 / WL;
  float hv[HV];
  {
    const int HPn = Pm->history_len * Pm->num_proprio;
    const float* hsrc = B.obs_history + (size_t)e * HPn;
#pragma unroll
    for (int t = 0; t < HV; ++t) {
      const int i = lane + WL * t;
      hv[t] = i < HPn ? hsrc[i] : 0.f;
    }
  }
  fill_uniforms<WL>(AR, seed, gid, step, 0, lane, rng_blocks(Pm));
  PH(12);
  const bool go2 = Pm->task_kind == LGX_TASK_GO2;
  if (lane == 0) {
    Scratch& x = s.x;
    float* root = s.root;
    float* cmd = s.cmd;
    const long long ep = s.ep_prev + 1;
    s.ep = ep;
    const float g[3] = {0.f, 0.f, -1.f};
    quat_rotate_inverse(root + 3, root + 7, x.blv);
    quat_rotate_inverse(root + 3, root + 10, x.bav);
    quat_rotate_inverse(root + 3, g, x.pg);
    x.roll = x.pitch = x.yaw = 0.f;
    x.ph[0] = x.ph[1] = x.ph[2] = x.ph[3] = 0.f;
    for (int f = 0; f < 4; ++f) { x.contact[f] = 0; x.feet_z[f] = 0.f; s.lc[f] = 0; s.lch[f] = 0.f; s.fat[f] = 0.f; }
    if (go2) {
      // update_feet_states go2.py:266-328
      float phase = trem((float)ep * Pm->dt, Pm->period) / Pm->period;
      float pfr = trem(phase + Pm->offset_fr, 1.0f), pbl = trem(phase + Pm->offset_bl, 1.0f);
      float pfl = trem(phase + Pm->offset_fl, 1.0f), pbr = trem(phase + Pm->offset_br, 1.0f);
      float msk = (nrm3(cmd[0], cmd[1], cmd[2]) < 0.2f) ? 0.0f : 1.0f;
      x.ph[0] = pfl * msk; x.ph[1] = pfr * msk; x.ph[2] = pbl * msk; x.ph[3] = pbr * msk;
      for (int f = 0; f < 4; ++f) {
        int lcf = s.lc_prev[f];
        float lch = s.lch_prev[f];
        int curc = s.cf[Pm->feet_idx[f]][2] > 1.0f;
        x.contact[f] = curc || lcf;
        s.lc[f] = curc;
        x.feet_z[f] = s.rbz[Pm->feet_idx[f]];
        s.lch[f] = x.contact[f] ? x.feet_z[f] : lch;
        if (B.feet_air_time) s.fat[f] = s.fat_prev[f];
      }
      // quaternion_to_euler go2.py:11-31
      float qx = root[3], qy = root[4], qz = root[5], qw = root[6];
      x.roll = atan2f(2.0f * (qw * qx + qy * qz), 1.0f - 2.0f * (qx * qx + qy * qy));
      x.pitch = asinf(clipf(2.0f * (qw * qy - qz * qx), -1.0f, 1.0f));
      x.yaw = atan2f(2.0f * (qw * qz + qx * qy), 1.0f - 2.0f * (qy * qy + qz * qz));
    }
    // _post_physics_step_callback go2.py:390-410
    if (ep % Pm->resample_interval == 0) resample_commands(Pm, B.command_ranges, cmd, stg_U(AR), S_CMD, root + 3);
    if (Pm->heading_command) {
      const float fwd[3] = {1.f, 0.f, 0.f};
      float f[3];
      quat_apply(root + 3, fwd, f);
      float heading = atan2f(f[1], f[0]);
      float gain = go2 ? Pm->heading_error_gain : 0.5f;
      cmd[2] = clipf(wrap_to_pi(cmd[3] - heading) * gain, -1.0f, 1.0f);
    }
    // command schedule (include/lgx.h, ABI 10): after the resample and the heading rule, so an
    // active segment's yaw rate stands; the env's row is read from global memory (Sh does not grow)
    if (B.cmd_step)
      scheduled_command(cmd, B.cmd_step + (size_t)e * LGX_CMD_SEGMENTS,
                        B.cmd_val + (size_t)e * LGX_CMD_SEGMENTS * 4, ep);
    if (Pm->push_robots && (step % (uint64_t)Pm->push_interval == 0)) {
      root[7] = rand_range(-Pm->max_push_vel_xy, Pm->max_push_vel_xy, stg_U(AR)[S_PUSH + 0]);
      root[8] = rand_range(-Pm->max_push_vel_xy, Pm->max_push_vel_xy, stg_U(AR)[S_PUSH + 1]);
    }
    // scheduled push (include/lgx.h, ABI 9): ep >= 1, so a push_step <= 0 never fires
    if (B.push_step && (long long)B.push_step[e] == ep) scheduled_push(root, B.push_dvel + (size_t)e * 3);
    // check_termination go2.py:186-204
    int reset = 0;
    for (int i = 0; i < Pm->n_termination; ++i) {
      const float* c = s.cf[Pm->termination_idx[i]];
      reset |= nrm3(c[0], c[1], c[2]) > 1.0f;
    }
    // a blown-up env (NaN/Inf guard) ends as a termination, never a time-out: its step is not
    // bootstrapped (ppo.py:166-167) and earns no reward (the stand-in state is not a real one)
    int tout = ep > Pm->max_episode_length && !s.blew;
    reset |= tout;
    reset |= x.pg[2] > 0.0f;
    if (Pm->parkour) reset |= root[2] < -1.0f;
    reset |= s.blew;  // NaN/Inf guard
    s.reset = reset;
    s.tout = tout;
    x.jump = s.jump_prev;  // set by the previous step's observations
  }
  __syncthreads();
  PH(13);
  get_heights<WL>(Pm, B, s, AR, lane);
  __syncthreads();
  joint_sums(Pm, B, s, AR, e, lane);
  __syncthreads();
  // compute_reward legged_robot.py:216-237: lane k evaluates term k (alphabetical order)
  const int K = Pm->num_reward_terms;
  const int KS = K + (Pm->has_termination_reward ? 1 : 0);
  for (int k = lane; k < K; k += WL)
    s.rterm[k] = s.blew ? 0.0f : reward_term(Pm, s, Pm->reward_ids[k]) * Pm->reward_scales[k];
  __syncthreads();
  const int reset = s.reset;
  if (lane == 0) {
    float rew = 0.0f;
    for (int k = 0; k < K; ++k) rew += s.rterm[k];  // sequential, the reference's order
    if (Pm->only_positive_rewards) rew = rew < 0.0f ? 0.0f : rew;
    if (Pm->has_termination_reward) {
      float v = (float)(reset && !s.tout && !s.blew) * Pm->termination_scale;
      rew += v;
      s.rterm[K] = v;
    }
    B.rew[e] = rew;
    B.reset[e] = (uint8_t)reset;
    B.time_out[e] = (uint8_t)s.tout;
    if (B.blew_up) B.blew_up[e] = (uint8_t)s.blew;
  }
  __syncthreads();
  for (int k = lane; k < KS; k += WL) {
    const float v = s.es[k] + s.rterm[k];
    s.es[k] = v;
    B.episode_sums[(size_t)e * KS + k] = v;
  }
  __syncthreads();
  PH(14);
  // scan model (include/lgx.h, ABI 17), SENSOR instances: the second lookup of an env with a map
  // offset uses the pose the height scan above used, which a reset replaces. (Like get_heights it
  // asks the mesh type at run time: lgx_post_physics runs a terrain on a TERRAIN = false instance.)
  float scan_pose[4] = {0.f, 0.f, 0.f, 1.f};
  if constexpr (SENSOR) {
    if (B.scan_offset) {
      scan_pose[0] = s.root[0]; scan_pose[1] = s.root[1];
      scan_pose[2] = s.root[5]; scan_pose[3] = s.root[6];
    }
  }
  // reset_idx (go2.py:207-263)
  if (reset) reset_env<WL>(Pm, B, s, AR, e, lane, true, false, true);

  // compute_observations go2.py:467-574 / legged_robot.py:240-273
  const int Pp = Pm->num_proprio, H = Pm->history_len;
  const Scratch& x = s.x;
  if (go2 && Pm->parkour && lane == 0) {
    int outl = 0;
    for (int i = 0; i < Pm->num_height_points; ++i) outl += fabsf(stg_heights(AR, Pm)[i]) > 0.1f;
    s.x.jump = (float)(outl >= 8);
  }
  for (int i = lane; i < Pp; i += WL) {
    float v;
    if (go2) {
      if (i < 3) v = x.bav[i] * Pm->obs_scale_ang_vel;
      else if (i == 3) v = x.roll;
      else if (i == 4) v = x.pitch;
      else if (i < 8) v = s.cmd[i - 5] * Pm->commands_scale[i - 5];
      else if (i < 8 + D) v = (s.th[i - 8] - Pm->default_dof_pos[i - 8]) * Pm->obs_scale_dof_pos;
      else if (i < 8 + 2 * D) v = s.thd[i - 8 - D] * Pm->obs_scale_dof_vel;
      else if (i < 8 + 2 * D + A) v = s.act[i - 8 - 2 * D];
      else {
        int q = i - (8 + 2 * D + A);  // sin/cos of FR, FL, BL, BR
        int leg = (q >> 1) == 0 ? 1 : ((q >> 1) == 1 ? 0 : (q >> 1));
        float p = 6.283185307179586f * x.ph[leg];
        v = (q & 1) ? cosf(p) : sinf(p);
      }
    } else {
      if (i < 3) v = x.blv[i] * Pm->obs_scale_lin_vel;
      else if (i < 6) v = x.bav[i - 3] * Pm->obs_scale_ang_vel;
      else if (i < 9) v = x.pg[i - 6];
      else if (i < 12) v = s.cmd[i - 9] * Pm->commands_scale[i - 9];
      else if (i < 12 + D) v = (s.th[i - 12] - Pm->default_dof_pos[i - 12]) * Pm->obs_scale_dof_pos;
      else if (i < 12 + 2 * D) v = s.thd[i - 12 - D] * Pm->obs_scale_dof_vel;
      else if (i < 12 + 2 * D + A) v = s.act[i - 12 - 2 * D];
      else v = clipf(s.root[2] - 0.5f - stg_heights(AR, Pm)[i - (12 + 2 * D + A)], -1.0f, 1.0f) * Pm->obs_scale_height;
    }
    // (the SENSOR instances stage the raw row here and form the modelled one in the pass below)
    if constexpr (!SENSOR)
      if (Pm->add_noise) v = v + obs_noise_term(stg_U(AR)[S_NOISE + i], Pm->noise_vec[i]);
    stg_cur(AR, Pm)[i] = v;
  }
  // Sensor model (include/lgx.h, ABI 15), in the SENSOR instances only: latency on the sensor
  // channels through the env's ring in global memory, then the noise term with the env's scale,
  // then the env's bias. Lane i re-reads the raw value it staged (its own LDS word: no barrier),
  // reads and then overwrites column i of the ring, consecutive lanes on consecutive words of a
  // row. No LDS beyond the staged row. Count and latency are per env: every lane of the env loads
  // the same word (a vector load; at two envs per wave uniform over a half-wave only). An env this
  // step reset starts at count 0, so its latency clamps to 0 and the count needs no zeroing here.
  int scan_c = 0;  // the scan model's copy of the count (ABI 17; the rings share it)
  if constexpr (SENSOR) {
    // rows of this episode in the ring (0 for an env this step reset) and the env's clamped latency
    int sens_c = 0, sens_d = 0;
    if (B.sensor_count) {
      sens_c = reset ? 0 : B.sensor_count[e];
      if (B.obs_delay) sens_d = sensor_delay_clamp(B.obs_delay[e], Pm->sensor_history_len, sens_c);
    }
    for (int i = lane; i < Pp; i += WL) {
      float v = stg_cur(AR, Pm)[i];
      if (B.sensor_history) {
        const int SK = Pm->sensor_history_len;
        float* ring = B.sensor_history + (size_t)e * SK * Pp;
        const float raw = v;
        if (sens_d > 0 && sensor_channel(go2, i, D, A)) v = ring[(size_t)sensor_ring_read_row(sens_c, sens_d, SK) * Pp + i];
        ring[(size_t)sensor_ring_write_row(sens_c, SK) * Pp + i] = raw;
      }
      v = sensor_noise_bias(v, Pm->add_noise != 0, Pm->add_noise ? stg_U(AR)[S_NOISE + i] : 0.f, Pm->noise_vec[i],
                            B.obs_noise_scale ? B.obs_noise_scale + e : nullptr,
                            B.obs_bias ? B.obs_bias + (size_t)e * Pp + i : nullptr);
      stg_cur(AR, Pm)[i] = v;
    }
    if (B.sensor_count && lane == 0) B.sensor_count[e] = sens_c + 1;
    scan_c = sens_c;
  }
  // stage the old history (obs[0:H*P]) in LDS; a reset env's history was zeroed (go2.py:238)
  float* hist_g = B.obs_history + (size_t)e * H * Pp;
  float* const hist = stg_hist(AR, Pm);
  const float* const cur = stg_cur(AR, Pm);
  const bool hl = hist_in_lds(Pm);
  const long long ep = s.ep;
  const float co = Pm->clip_obs;
  float* obs = B.obs + (size_t)e * Pm->num_obs;
  float* cr = B.critic ? B.critic + (size_t)e * Pm->num_critic : nullptr;
  if (hl) {
#pragma unroll
    for (int t = 0; t < HV; ++t) {
      const int i = lane + WL * t;
      if (i < H * Pp) hist[i] = reset ? 0.f : hv[t];
    }
    for (int i = lane + WL * HV; i < H * Pp; i += WL) hist[i] = reset ? 0.f : hist_g[i];
  }
  __syncthreads();
  if (hl) {
    for (int i = lane; i < H * Pp; i += WL) {
      float v = clipf(hist[i], -co, co);
      obs[i] = v;
      if (go2 && cr) cr[i] = v;
    }
  } else {
    // long history, shifted in place: entry i of the old history goes to obs[i], and the new
    // history's entry i is old entry i + P (or the current observation, go2.py:570-574).
    // Chunks of 64 in increasing i: a chunk reads old entries >= its own first index (P >= 64)
    // and writes only its own 64, after its reads are consumed — no entry is overwritten
    // before it is read.
    const int HP = H * Pp, HP1 = (H - 1) * Pp;
#pragma unroll
    for (int t = 0; t < (MAXHIST + WL - 1) / WL; ++t) {
      const int i = lane + WL * t;
      if (WL * t >= HP) break;
      if (i < HP) {
        const float old = reset ? 0.f : (t < HV ? hv[t < HV ? t : 0] : hist_g[i]);
        const float v = clipf(old, -co, co);
        obs[i] = v;
        if (go2 && cr) cr[i] = v;
        const float nv = (ep <= 1) ? cur[i % Pp] : (i < HP1 ? hist_g[i + Pp] : cur[i - HP1]);
        hist_g[i] = nv;
      }
    }
  }
  for (int i = lane; i < Pp; i += WL) {
    float v = clipf(cur[i], -co, co);
    obs[H * Pp + i] = v;
    if (go2 && cr) cr[H * Pp + i] = v;
  }
  if (go2) {
    const int NO = Pm->num_obs;
    // priv = [mass params (4), friction, kp-1 (D), kd-1 (D)]
    for (int i = lane; i < Pm->num_priv; i += WL) {
      float v;
      if (i < 4) v = i == 0 ? s.madd : s.cadd[i - 1];  // mass_params row, staged at kernel start
      else if (i == 4) v = s.fric;
      else if (i < 5 + D) v = s.kpm[i - 5] - 1.0f;
      else v = s.kdm[i - 5 - D] - 1.0f;
      v = clipf(v, -co, co);
      B.priv[(size_t)e * Pm->num_priv + i] = v;
      if (cr) cr[NO + i] = v;
    }
    if (lane < 3) {
      float v = clipf(x.blv[lane] * Pm->obs_scale_lin_vel, -co, co);
      B.est[(size_t)e * Pm->num_est + lane] = v;
      if (cr) cr[NO + Pm->num_priv + lane] = v;
    }
    if constexpr (!SENSOR) {
      for (int i = lane; i < Pm->num_scan; i += WL) {
        float v = clipf(s.root[2] - 0.3f - stg_heights(AR, Pm)[i], -1.0f, 1.0f);
        B.scan[(size_t)e * Pm->num_scan + i] = v;
        if (cr) cr[NO + Pm->num_priv + 3 + i] = clipf(v, -co, co);
      }
    } else {
      // Height-scan model (include/lgx.h, ABI 17): per point the raw value (from a second terrain
      // lookup for an env whose map is shifted in xy), the latency through the env's ring in
      // global memory, then scan_point_model. The critic's copy stays the clean value. Lane i has
      // points i, i + WL, ...: ring traffic is consecutive lanes on consecutive words of a row, and
      // each lane reads and then overwrites its own column. No LDS beyond the staged heights. The
      // env's four rows are the same word for every lane of the env (vector loads). A lane
      // recomputes the Philox block of its point (the four lanes of a block would otherwise
      // exchange it across a divergent branch); an env without noise and dropout draws nothing.
      const int S = Pm->num_scan;
      const float amp = B.scan_noise ? B.scan_noise[e] : 0.f;
      const float drop_p = B.scan_dropout ? B.scan_dropout[(size_t)e * 2] : 0.f;
      const float fill = B.scan_dropout ? B.scan_dropout[(size_t)e * 2 + 1] : 0.f;
      float dx = 0.f, dy = 0.f, dz = 0.f;
      if (B.scan_offset) {
        dx = B.scan_offset[(size_t)e * 3];
        dy = B.scan_offset[(size_t)e * 3 + 1];
        dz = B.scan_offset[(size_t)e * 3 + 2];
      }
      const bool second = (dx != 0.f || dy != 0.f) && Pm->mesh_type != LGX_MESH_PLANE && B.height_samples != nullptr;
      float qy[4] = {0.f, 0.f, 0.f, 1.f};
      if (second) scan_yaw_quat(scan_pose[2], scan_pose[3], qy);
      const int SK = Pm->sensor_history_len;
      const int scan_d = B.scan_delay ? sensor_delay_clamp(B.scan_delay[e], SK, scan_c) : 0;
      for (int i = lane; i < S; i += WL) {
        const float clean = scan_raw(s.root[2], stg_heights(AR, Pm)[i]);
        float raw = clean;
        if (second)
          raw = scan_raw(s.root[2], scan_point_height(Pm, B.height_samples, qy, scan_pose, Pm->height_points[i][0] + dx,
                                                      Pm->height_points[i][1] + dy));
        float v = raw;
        if (B.scan_history) {
          float* ring = B.scan_history + (size_t)e * SK * S;
          if (scan_d > 0) v = ring[(size_t)sensor_ring_read_row(scan_c, scan_d, SK) * S + i];
          ring[(size_t)sensor_ring_write_row(scan_c, SK) * S + i] = raw;
        }
        const float u = amp != 0.f ? scan_uniform(seed, gid, step, i) : 0.f;
        const float ud = drop_p > 0.f ? scan_uniform(seed, gid, step, LGX_MAX_HEIGHT_POINTS + i) : 0.f;
        B.scan[(size_t)e * S + i] = scan_point_model(v, amp, u, dz, drop_p, ud, fill);
        if (cr) cr[NO + Pm->num_priv + 3 + i] = clipf(clean, -co, co);
      }
    }
  }
  // history update go2.py:570-574 (the long-history path wrote it above)
  if (hl)
    for (int i = lane; i < H * Pp; i += WL) {
      float v = (ep <= 1) ? cur[i % Pp] : (i < (H - 1) * Pp ? hist[i + Pp] : cur[i - (H - 1) * Pp]);
      hist_g[i] = v;
    }
  // last_* copies go2.py:380-384 and state write-back
  if (lane < A) B.last_actions[(size_t)e * A + lane] = s.act[lane];
  if (B.action_history && lane < A) {  // each lane its own column: the substeps' reads are done
    const int AH = Pm->action_history_len;
    action_history_push(B.action_history + (size_t)e * AH * A, AH, A, lane, s.act[lane], reset != 0);
  }
  if (lane < D) {
    B.last_dof_vel[(size_t)e * D + lane] = s.thd[lane];
    B.last_torques[(size_t)e * D + lane] = s.tau[lane];
    B.dof_state[((size_t)e * D + lane) * 2] = s.th[lane];
    B.dof_state[((size_t)e * D + lane) * 2 + 1] = s.thd[lane];
  }
  if (lane < 6) B.last_root_vel[e * 6 + lane] = s.root[7 + lane];
  if (lane < 3) {
    B.last_base_lin_vel[e * 3 + lane] = x.blv[lane];
    if (B.base_lin_vel) B.base_lin_vel[e * 3 + lane] = x.blv[lane];
    if (B.base_ang_vel) B.base_ang_vel[e * 3 + lane] = x.bav[lane];
    if (B.projected_gravity) B.projected_gravity[e * 3 + lane] = x.pg[lane];
  }
  if (lane < 13) root_g[lane] = s.root[lane];
  if (lane < 4) B.commands[e * 4 + lane] = s.cmd[lane];
  if (go2 && lane < Pm->num_feet && !reset) {
    B.last_contacts[e * Pm->num_feet + lane] = (uint8_t)s.lc[lane];
    B.last_contact_heights[e * Pm->num_feet + lane] = s.lch[lane];
    if (B.feet_air_time) B.feet_air_time[e * Pm->num_feet + lane] = s.fat[lane];
  }
  if (lane == 0) B.episode_length[e] = ep;
  if (B.rpy_phase && lane < 8) {
    float v = lane == 0 ? x.roll : lane == 1 ? x.pitch : lane == 2 ? x.yaw : lane < 7 ? x.ph[lane - 3] : x.jump;
    B.rpy_phase[e * 8 + lane] = v;
  }
  if (B.measured_heights)
    for (int i = lane; i < Pm->num_height_points; i += WL)
      B.measured_heights[(size_t)e * Pm->num_height_points + i] = stg_heights(AR, Pm)[i];
#ifdef LGX_PHASE_CLOCK
  __syncthreads();
  PH(15);
  __syncthreads();
  if (lane == 0) {  // where the wave ran: HW_ID (wave, SIMD, CU, SE fields) and XCC_ID
    s.phacc[18] = __builtin_amdgcn_s_getreg(4 | (31 << 11));
    s.phacc[19] = __builtin_amdgcn_s_getreg(20 | (31 << 11));
  }
  __syncthreads();
  if (g_phase_out && lane < NPH) g_phase_out[(size_t)e * NPH + lane] = s.phacc[lane];
#endif
}

// BaseTask.reset -> reset_idx(env_ids) outside a step (RNG stream 1)
__global__ __launch_bounds__(64) void reset_kernel(const lgx_task_params* __restrict__ Pm,
                                                   const lgx_buffers* __restrict__ Bp,
                                                   const uint8_t* __restrict__ mask, uint64_t seed, uint64_t call) {
  __shared__ Sh s;
  const lgx_buffers& B = *Bp;
  const int e = blockIdx.x;
  const int lane = threadIdx.x;
  if (!mask[e]) return;
  const int D = Pm->num_dof;
  fill_uniforms<64>(lgx_dyn, seed, (uint32_t)(Pm->env_id_offset + e), call, 1, lane, rng_blocks(Pm));
  if (lane < 13) s.root[lane] = B.root_states[(size_t)e * 13 + lane];
  if (lane < 4) s.cmd[lane] = B.commands[e * 4 + lane];
  __syncthreads();
  // an external reset (BaseTask.reset -> reset_idx) only exists once the env is built,
  // i.e. with init_done set: the terrain curriculum applies (legged_robot.py:551-552)
  reset_env<64>(Pm, B, s, lgx_dyn, e, lane, true, true, false);
  if (B.sensor_count && lane == 0) B.sensor_count[e] = 0;  // sensor model (ABI 15): the new episode's ring is empty
  if (lane < 13) B.root_states[(size_t)e * 13 + lane] = s.root[lane];
  if (lane < D) {
    B.dof_state[((size_t)e * D + lane) * 2] = s.th[lane];
    B.dof_state[((size_t)e * D + lane) * 2 + 1] = s.thd[lane];
  }
  if (lane < 4) B.commands[e * 4 + lane] = s.cmd[lane];
  if (lane == 0) { B.episode_length[e] = s.ep; B.reset[e] = 1; }
}

}  // namespace lgx

// ============================================================== C ABI
#include <stdio.h>

#include <initializer_list>
#include <string>

struct lgx_env {
  lgx_model model;
  lgx_task_params params;
  lgx_buffers buffers;
  lgx_model* d_model = nullptr;
  lgx_task_params* d_params = nullptr;
  lgx_buffers* d_buffers = nullptr;  // device copy of `buffers` (kernels read pointers from it)
  int device = 0;
  bool host = false;         // device < 0: the host backend (lgx_env_host.cpp), host buffers
  bool bound = false;
  bool stats_clean = false;  // episode_stats zeroed by lgx_episode_extras and not written since
  int epw = 0;               // envs per wave (lgx_set_envs_per_wave; 0: default)
  std::string err;
};

static int fail(lgx_env* env, const std::string& msg) {
  if (env) env->err = msg;
  return -1;
}

#define HIP_OK(call)                                                                   \
  do {                                                                                 \
    hipError_t _e = (call);                                                            \
    if (_e != hipSuccess) return fail(env, std::string(#call ": ") + hipGetErrorString(_e)); \
  } while (0)

extern "C" {

int32_t lgx_abi_version(void) { return LGX_ABI_VERSION; }
int64_t lgx_sizeof_model(void) { return (int64_t)sizeof(lgx_model); }
int64_t lgx_sizeof_task_params(void) { return (int64_t)sizeof(lgx_task_params); }
int64_t lgx_sizeof_buffers(void) { return (int64_t)sizeof(lgx_buffers); }

int lgx_create(const lgx_model* model, const lgx_task_params* params, int32_t device, lgx_env** out) {
  if (!model || !params || !out) return -2;
  lgx_env* env = new lgx_env();
  *out = env;
  env->model = *model;
  env->params = *params;
  env->device = device;
  if (params->abi_version != LGX_ABI_VERSION) return fail(env, "ABI version mismatch");
  // the kernel's structured solver assumes base + 4 chains of 3 revolute joints
  if (model->num_links != lgx::NL || params->num_dof != lgx::NJ)
    return fail(env, "model must be a floating base with 4 chains of 3 joints (13 links, 12 dof)");
  for (int l = 0; l < 4; ++l)
    for (int i = 0; i < 3; ++i) {
      int k = 1 + 3 * l + i;
      int expect = i == 0 ? 0 : k - 1;
      if (model->link_parent[k] != expect) return fail(env, "link tree is not 4 serial chains of 3");
    }
  if (model->num_candidates > LGX_MAX_CANDIDATES || model->num_bodies > LGX_MAX_BODIES)
    return fail(env, "too many contact candidates or bodies");
  if (params->history_len * params->num_proprio > lgx::MAXHIST) return fail(env, "history too long");
  if (params->num_proprio > LGX_MAX_PROPRIO || params->num_height_points > LGX_MAX_HEIGHT_POINTS)
    return fail(env, "observation too large");
  if (params->num_reward_terms + 1 > 64) return fail(env, "too many reward terms");
  if (params->action_history_len < 0 || params->action_history_len > LGX_MAX_ACTION_HISTORY)
    return fail(env, "action_history_len outside 0..LGX_MAX_ACTION_HISTORY");
  if (params->sensor_history_len < 0 || params->sensor_history_len > LGX_MAX_SENSOR_HISTORY)
    return fail(env, "sensor_history_len outside 0..LGX_MAX_SENSOR_HISTORY");
  // observation layout the step writes (go2.py:467-574 / legged_robot.py:240-273): obs =
  // [history (H x P) | current (P)]; Go2 critic = [obs | priv | est (3) | scan]. A config whose
  // declared sizes disagree (the reference's anymal_c_flat: 48-wide obs, 235-wide proprio)
  // fails here — the reference fails at its first compute_observations (torch.cat shapes).
  {
    const lgx_task_params& p = *params;
    const int D = p.num_dof, A = p.num_actions;
    const int want_p = p.task_kind == LGX_TASK_GO2 ? 8 + 2 * D + A + 8
                                                   : 12 + 2 * D + A + (p.measure_heights ? p.num_height_points : 0);
    char msg[256];
    if (p.num_proprio != want_p) {
      snprintf(msg, sizeof msg, "num_proprio %d != %d (the observation terms of this task)", p.num_proprio, want_p);
      return fail(env, msg);
    }
    if (p.num_obs != (p.history_len + 1) * p.num_proprio) {
      snprintf(msg, sizeof msg, "num_observations %d != (history_buffer_length + 1) * num_proprio = %d", p.num_obs,
               (p.history_len + 1) * p.num_proprio);
      return fail(env, msg);
    }
    if (p.task_kind == LGX_TASK_GO2 &&
        (p.num_priv != 5 + 2 * D || p.num_est != 3 || p.num_scan > p.num_height_points ||
         p.num_critic != p.num_obs + p.num_priv + p.num_est + p.num_scan))
      return fail(env, "Go2 privileged/estimated/scan/critic observation sizes do not match the step's layout");
    if (p.num_feet > LGX_MAX_FEET) return fail(env, "too many feet");
  }
  if (device < 0) {  // host backend: no device state; every buffer is host memory
    env->host = true;
    return 0;
  }
  HIP_OK(hipSetDevice(device));
  HIP_OK(hipMalloc(&env->d_model, sizeof(lgx_model)));
  HIP_OK(hipMalloc(&env->d_params, sizeof(lgx_task_params)));
  HIP_OK(hipMalloc(&env->d_buffers, sizeof(lgx_buffers)));
  HIP_OK(hipMemcpy(env->d_model, model, sizeof(lgx_model), hipMemcpyHostToDevice));
  HIP_OK(hipMemcpy(env->d_params, params, sizeof(lgx_task_params), hipMemcpyHostToDevice));
  return 0;
}

int lgx_bind(lgx_env* env, const lgx_buffers* b) {
  if (!env || !b) return -2;
  static const char* required[] = {"root_states", "dof_state", "contact_forces", "rigid_body_states", "actions_in",
                                   "actions", "torques", "last_actions", "last_dof_vel", "last_root_vel",
                                   "last_base_lin_vel", "last_torques", "commands", "episode_length",
                                   "episode_sums", "obs_history", "obs", "rew", "reset", "time_out", "env_origins"};
  const void* ptrs[] = {b->root_states, b->dof_state, b->contact_forces, b->rigid_body_states, b->actions_in,
                        b->actions, b->torques, b->last_actions, b->last_dof_vel, b->last_root_vel,
                        b->last_base_lin_vel, b->last_torques, b->commands, b->episode_length,
                        b->episode_sums, b->obs_history, b->obs, b->rew, b->reset, b->time_out, b->env_origins};
  for (size_t i = 0; i < sizeof(ptrs) / sizeof(ptrs[0]); ++i)
    if (!ptrs[i]) return fail(env, std::string("lgx_bind: required buffer missing: ") + required[i]);
  if (env->params.task_kind == LGX_TASK_GO2) {
    if (!b->priv || !b->est || !b->scan || !b->critic || !b->last_contacts || !b->last_contact_heights ||
        !b->mass_params || !b->friction)
      return fail(env, "lgx_bind: Go2 task needs priv/est/scan/critic/last_contacts/last_contact_heights/mass_params/friction");
  }
  if (env->params.mesh_type != LGX_MESH_PLANE) {
    if (!b->height_samples || !b->terrain_mesh)
      return fail(env, "lgx_bind: heightfield/trimesh terrain needs height_samples and terrain_mesh");
    if (env->params.hf_rows < 2 || env->params.hf_cols < 2) return fail(env, "lgx_bind: terrain smaller than 2x2");
  }
  if (env->params.actuator_net && (!b->sea_hidden || !b->sea_cell))
    return fail(env, "lgx_bind: the actuator network needs sea_hidden/sea_cell [2, N*D, 8]");
  if (env->params.actuator_net &&
      ((reinterpret_cast<uintptr_t>(b->sea_hidden) | reinterpret_cast<uintptr_t>(b->sea_cell)) & 15))
    return fail(env, "lgx_bind: sea_hidden/sea_cell must be 16-byte aligned");
  if (b->action_delay && (!b->action_history || env->params.action_history_len <= 0))
    return fail(env, "lgx_bind: action_delay needs action_history and params.action_history_len > 0");
  if (b->action_history && env->params.action_history_len <= 0)
    return fail(env, "lgx_bind: action_history with params.action_history_len = 0");
  if (b->obs_delay && (!b->sensor_history || !b->sensor_count || env->params.sensor_history_len <= 0))
    return fail(env, "lgx_bind: obs_delay needs sensor_history, sensor_count and params.sensor_history_len > 0");
  if (b->sensor_history && !b->sensor_count) return fail(env, "lgx_bind: sensor_history needs sensor_count");
  if (b->sensor_count && !b->sensor_history && !b->scan_history)
    return fail(env, "lgx_bind: sensor_count needs sensor_history or scan_history");
  if ((b->scan_noise || b->scan_dropout || b->scan_offset || b->scan_delay || b->scan_history) &&
      (env->params.task_kind != LGX_TASK_GO2 || env->params.num_scan <= 0))
    return fail(env, "lgx_bind: the scan model needs the Go2 task kind and params.num_scan > 0");
  if (b->scan_delay && (!b->scan_history || !b->sensor_count || env->params.sensor_history_len <= 0))
    return fail(env, "lgx_bind: scan_delay needs scan_history, sensor_count and params.sensor_history_len > 0");
  if (b->scan_history && !b->sensor_count) return fail(env, "lgx_bind: scan_history needs sensor_count");
  if (b->scan_history && env->params.sensor_history_len <= 0)
    return fail(env, "lgx_bind: scan_history with params.sensor_history_len = 0");
  if (b->sensor_history && env->params.sensor_history_len <= 0)
    return fail(env, "lgx_bind: sensor_history with params.sensor_history_len = 0");
  if (b->force_window && !b->force_vec) return fail(env, "lgx_bind: force_window without force_vec");
  if (b->force_vec && !b->force_window) return fail(env, "lgx_bind: force_vec without force_window");
  if (b->push_step && !b->push_dvel) return fail(env, "lgx_bind: push_step without push_dvel");
  if (b->push_dvel && !b->push_step) return fail(env, "lgx_bind: push_dvel without push_step");
  if (b->cmd_step && !b->cmd_val) return fail(env, "lgx_bind: cmd_step without cmd_val");
  if (b->cmd_val && !b->cmd_step) return fail(env, "lgx_bind: cmd_val without cmd_step");
  if (env->params.curriculum && (!b->terrain_levels || !b->terrain_types || !b->terrain_origins))
    return fail(env, "lgx_bind: terrain curriculum needs terrain_levels/terrain_types/terrain_origins");
  env->buffers = *b;
  if (env->host) {
    env->bound = true;
    env->stats_clean = false;
    return 0;
  }
  HIP_OK(hipSetDevice(env->device));
  HIP_OK(hipMemcpy(env->d_buffers, b, sizeof(lgx_buffers), hipMemcpyHostToDevice));
  env->bound = true;
  env->stats_clean = false;
  return 0;
}

static int launch_step(lgx_env* env, uint64_t seed, uint64_t step, const uint64_t* step_dev, void* stream,
                       bool physics) {
  if (!env) return -2;
  if (!env->bound) return fail(env, "lgx_step before lgx_bind");
  hipStream_t st = (hipStream_t)stream;
  const int N = env->params.num_envs;
  const int KS = env->params.num_reward_terms + (env->params.has_termination_reward ? 1 : 0);
  if (env->host) {
    if (env->buffers.episode_stats && !env->stats_clean)
      for (int k = 0; k <= KS; ++k) env->buffers.episode_stats[k] = 0.f;
    env->stats_clean = false;
    lgxh::step(&env->model, &env->params, &env->buffers, seed, step_dev ? *step_dev : step, physics);
    return 0;
  }
  if (env->buffers.episode_stats && !env->stats_clean)
    HIP_OK(hipMemsetAsync(env->buffers.episode_stats, 0, sizeof(float) * (KS + 1), st));
  env->stats_clean = false;
  // compiled variants: the plane/PD path (the benchmark) carries no terrain or LSTM code. Two
  // envs per wave (EPW 2: 32 lanes each, lgx_env.hip grp_of_lane) by default on the plane with an
  // even env count (measured: Go2 4096 envs 184 -> 177 us); on a trimesh the one-env kernel is
  // faster (go2_parkour 8192 envs: 423 vs 491 us), so there EPW 2 only when asked for
  // (lgx_set_envs_per_wave); never with the actuator net (its LSTM lanes need the whole wave).
  // LGX_ENVS_PER_WAVE=1 selects one env per wave (A/B, tests)
  const bool terrain = env->params.mesh_type != LGX_MESH_PLANE, actnet = env->params.actuator_net != 0;
  static const int epw_env = [] {
    const char* v = LGX_DEV_KNOB("LGX_ENVS_PER_WAVE");
    return v && atoi(v) == 1 ? 1 : 2;
  }();
  const int want = env->epw ? env->epw : (terrain ? 1 : epw_env);
  const int epw = (!actnet && N % 2 == 0 && want == 2) ? 2 : 1;
  // the sensor model's code lives in instances of its own (SENSOR), chosen from the bound pointers:
  // with none of them bound the step runs the code it ran before ABI 15
  const lgx_buffers& hb = env->buffers;
  // (the scan model of ABI 17 lives in the same instances)
  const bool sensor = hb.obs_noise_scale || hb.obs_bias || hb.sensor_history || hb.scan_noise || hb.scan_dropout ||
                      hb.scan_offset || hb.scan_delay || hb.scan_history;
  // and so does the external force's (FORCE; it acts in the physics: the other instances have none)
  const bool force = hb.force_window != nullptr;
#define LGX_STEP_KERNEL(SENSOR, FORCE)                                                                       \
  (epw == 2 ? (!physics ? lgx::env_step_kernel<false, false, false, 2, SENSOR, false>                        \
                        : (terrain ? lgx::env_step_kernel<true, true, false, 2, SENSOR, FORCE>               \
                                   : lgx::env_step_kernel<true, false, false, 2, SENSOR, FORCE>))            \
   : !physics ? lgx::env_step_kernel<false, false, false, 1, SENSOR, false>                                  \
   : actnet   ? (terrain ? lgx::env_step_kernel<true, true, true, 1, SENSOR, FORCE>                          \
                         : lgx::env_step_kernel<true, false, true, 1, SENSOR, FORCE>)                        \
              : (terrain ? lgx::env_step_kernel<true, true, false, 1, SENSOR, FORCE>                         \
                         : lgx::env_step_kernel<true, false, false, 1, SENSOR, FORCE>))
  auto kern = sensor ? (force ? LGX_STEP_KERNEL(true, true) : LGX_STEP_KERNEL(true, false))
                     : (force ? LGX_STEP_KERNEL(false, true) : LGX_STEP_KERNEL(false, false));
#undef LGX_STEP_KERNEL
  const size_t dyn = sizeof(float) * (size_t)lgx::arena_floats(env->params) * epw;
  hipLaunchKernelGGL(kern, dim3(N / epw), dim3(64), dyn, st, env->d_model, env->d_params, env->d_buffers, seed, step,
                     step_dev);
  HIP_OK(hipGetLastError());
  return 0;
}

int lgx_set_envs_per_wave(lgx_env* env, int32_t envs_per_wave) {
  if (!env) return -2;
  if (envs_per_wave < 0 || envs_per_wave > 2) return fail(env, "lgx_set_envs_per_wave: 0, 1 or 2");
  env->epw = envs_per_wave;
  return 0;
}

int lgx_step(lgx_env* env, uint64_t seed, uint64_t step_counter, void* hip_stream) {
  return launch_step(env, seed, step_counter, nullptr, hip_stream, true);
}

int lgx_step_dev(lgx_env* env, uint64_t seed, const uint64_t* d_step_counter, void* hip_stream) {
  if (!d_step_counter) return fail(env, "lgx_step_dev: null step counter");
  return launch_step(env, seed, 0, d_step_counter, hip_stream, true);
}

int lgx_post_physics(lgx_env* env, uint64_t seed, uint64_t step_counter, void* hip_stream) {
  return launch_step(env, seed, step_counter, nullptr, hip_stream, false);
}

int lgx_physics(lgx_env* env, void* hip_stream) {
  (void)hip_stream;
  return fail(env, "lgx_physics: use lgx_step (physics is fused with the post-physics pass)");
}

int lgx_reset_envs(lgx_env* env, const uint8_t* env_mask, uint64_t seed, uint64_t reset_call, void* hip_stream) {
  if (!env) return -2;
  if (!env->bound) return fail(env, "lgx_reset_envs before lgx_bind");
  if (!env_mask) return fail(env, "lgx_reset_envs: env_mask is NULL");
  hipStream_t st = (hipStream_t)hip_stream;
  const int KS = env->params.num_reward_terms + (env->params.has_termination_reward ? 1 : 0);
  if (env->host) {
    if (env->buffers.episode_stats && !env->stats_clean)
      for (int k = 0; k <= KS; ++k) env->buffers.episode_stats[k] = 0.f;
    env->stats_clean = false;
    lgxh::reset(&env->params, &env->buffers, env_mask, seed, reset_call);
    return 0;
  }
  if (env->buffers.episode_stats && !env->stats_clean)
    HIP_OK(hipMemsetAsync(env->buffers.episode_stats, 0, sizeof(float) * (KS + 1), st));
  env->stats_clean = false;
  const size_t dyn = sizeof(float) * (size_t)lgx::arena_floats(env->params);
  hipLaunchKernelGGL(lgx::reset_kernel, dim3(env->params.num_envs), dim3(64), dyn, st, env->d_params,
                     env->d_buffers, env_mask, seed, reset_call);
  HIP_OK(hipGetLastError());
  return 0;
}

namespace lgx {
// extras['episode'] / extras['time_outs'] (go2.py:246-263, Appendix B Q5 stale values):
// one block; thread k < K forms the episode mean of reward term k, the block reduces
// any(reset) and the mean terrain level, then time_outs is refreshed when any env reset.
// The statistics are consumed (zeroed for the next step, which then needs no memset) and
// the device step counter, if given, advances for the next lgx_step_dev.
__global__ __launch_bounds__(1024) void extras_kernel(float* __restrict__ stats, uint64_t* __restrict__ step_dev,
                                                      int K, float inv_T, int N,
                                                      const uint8_t* __restrict__ reset,
                                                      const uint8_t* __restrict__ time_out,
                                                      const int64_t* __restrict__ levels, float* __restrict__ means,
                                                      float* __restrict__ level_mean, uint8_t* __restrict__ time_outs) {
  __shared__ int any_s;
  __shared__ double lsum[16];
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  if (tid == 0) any_s = 0;
  __syncthreads();
  const float cnt = stats[K];
  if (tid < K && cnt > 0.f) means[tid] = stats[tid] / cnt * inv_T;
  int any = 0;
  double ls = 0.0;
  for (int i = tid; i < N; i += blockDim.x) {
    if (reset) any |= reset[i];
    if (levels) ls += (double)levels[i];
  }
  if (reset && __any(any)) {
    if (lane == 0) atomicOr(&any_s, 1);
  }
  if (levels) {
    for (int o = 32; o > 0; o >>= 1) ls += __shfl_down(ls, o, 64);
    if (lane == 0) lsum[wv] = ls;
  }
  __syncthreads();
  if (tid <= K) stats[tid] = 0.f;  // every thread read cnt before the barrier
  if (tid == 0 && step_dev) *step_dev += 1;
  if (levels && tid == 0 && cnt > 0.f) {
    double t = 0.0;
    for (int w = 0; w < (int)(blockDim.x >> 6); ++w) t += lsum[w];
    *level_mean = (float)(t / N);
  }
  if (time_outs && any_s)
    for (int i = tid; i < N; i += blockDim.x) time_outs[i] = time_out[i];
}
}  // namespace lgx

int lgx_episode_extras(lgx_env* env, float* means, float* level_mean, uint8_t* time_outs, uint64_t* step_dev,
                       void* hip_stream) {
  if (!env) return -2;
  if (!env->bound) return fail(env, "lgx_episode_extras before lgx_bind");
  const lgx_buffers& b = env->buffers;
  if (!b.episode_stats || !means) return fail(env, "lgx_episode_extras: episode_stats and means are required");
  if (level_mean && !b.terrain_levels) return fail(env, "lgx_episode_extras: level_mean needs terrain_levels");
  if (time_outs && (!b.reset || !b.time_out)) return fail(env, "lgx_episode_extras: time_outs needs reset/time_out");
  const int KS = env->params.num_reward_terms + (env->params.has_termination_reward ? 1 : 0);
  if (KS + 1 > 1024) return fail(env, "lgx_episode_extras: too many reward terms");
  if (env->host) {
    lgxh::episode_extras(&env->params, &b, means, level_mean, time_outs, step_dev);
    env->stats_clean = true;
    return 0;
  }
  hipStream_t st = (hipStream_t)hip_stream;
  // torch divides a tensor by a Python scalar as a multiply by the fp32 reciprocal
  hipLaunchKernelGGL(lgx::extras_kernel, dim3(1), dim3(1024), 0, st, b.episode_stats, step_dev, KS,
                     1.0f / env->params.max_episode_length_s, env->params.num_envs, time_outs ? b.reset : nullptr,
                     b.time_out, level_mean ? b.terrain_levels : nullptr, means, level_mean, time_outs);
  HIP_OK(hipGetLastError());
  env->stats_clean = true;
  return 0;
}

namespace lgx {
// update_command_curriculum (go2.py:80-107 / legged_robot.py:580-591) after a step: one block.
// The mean runs over the envs reset in this step (reset_idx's env_ids); their pre-reset
// tracking_lin_vel sums were left in curriculum_vals by the step kernel. When the range
// changes, the reset envs' commands are resampled again from the same uniforms with the new
// range (reset_idx resamples after the curriculum, go2.py:222-230) and the command entries of
// their observation rows are rewritten (a reset env's history is zero in obs and all copies of
// the current observation in obs_history, go2.py:570-574).
__global__ __launch_bounds__(1024) void curriculum_kernel(const lgx_task_params* __restrict__ Pm,
                                                          const lgx_buffers* __restrict__ Bp, uint64_t seed,
                                                          uint64_t step_arg, const uint64_t* __restrict__ step_dev,
                                                          const double* __restrict__ global_sc) {
  const lgx_buffers& B = *Bp;
  const uint64_t step = step_dev ? *step_dev : step_arg;
  if (step % (uint64_t)Pm->max_episode_length != 0) return;
  __shared__ double red_s[16], red_c[16];
  __shared__ int changed;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6, N = Pm->num_envs;
  double sm = 0.0, ct = 0.0;
  if (!global_sc)
    for (int i = tid; i < N; i += blockDim.x)
      if (B.reset[i]) { sm += (double)B.curriculum_vals[i]; ct += 1.0; }
  for (int o = 32; o > 0; o >>= 1) { sm += __shfl_down(sm, o, 64); ct += __shfl_down(ct, o, 64); }
  if (lane == 0) { red_s[wv] = sm; red_c[wv] = ct; }
  __syncthreads();
  if (tid == 0) {
    double S = 0.0, Cn = 0.0;
    if (global_sc) { S = global_sc[0]; Cn = global_sc[1]; }
    else
      for (int w = 0; w < (int)(blockDim.x >> 6); ++w) { S += red_s[w]; Cn += red_c[w]; }
    changed = curriculum_update_ranges(Pm, B, S, Cn);
  }
  __syncthreads();
  if (!changed) return;
  for (int e = tid; e < N; e += blockDim.x)
    if (B.reset[e]) curriculum_rewrite_env(Pm, B, seed, step, e);
}
}  // namespace lgx

int lgx_command_curriculum(lgx_env* env, uint64_t seed, uint64_t step_counter, const uint64_t* d_step_counter,
                           const double* global_sum_count, void* hip_stream) {
  if (!env) return -2;
  if (!env->bound) return fail(env, "lgx_command_curriculum before lgx_bind");
  const lgx_buffers& b = env->buffers;
  if (!env->params.command_curriculum) return fail(env, "lgx_command_curriculum: params.command_curriculum is 0");
  if (!b.command_ranges || !b.curriculum_vals || !b.reset || !b.commands || !b.obs || !b.obs_history)
    return fail(env, "lgx_command_curriculum: command_ranges, curriculum_vals, reset, commands, obs, obs_history "
                     "must be bound");
  if (env->host) {
    lgxh::command_curriculum(&env->params, &b, seed, d_step_counter ? *d_step_counter : step_counter,
                             global_sum_count);
    return 0;
  }
  hipLaunchKernelGGL(lgx::curriculum_kernel, dim3(1), dim3(1024), 0, (hipStream_t)hip_stream, env->d_params,
                     env->d_buffers, seed, step_counter, d_step_counter, global_sum_count);
  HIP_OK(hipGetLastError());
  return 0;
}

// ------------------------------------------------------------------ policy evaluation (ABI 7)
namespace lgx {
struct EvalArgs {
  const float* commands;
  const float* lin_vel;
  const float* ang_vel;
  const float* torques;
  const float* dof_state;
  const float* contact;
  const uint8_t* reset;
  const uint8_t* time_out;
  const uint8_t* blew_up;  // optional
  float* acc;
  uint8_t* status;
  int N, D, NB, nfeet;
  int feet[LGX_MAX_FEET];
  float dt;
  // push recovery (ABI 9): push_rec NULL = none of these is read
  const float* pg;
  const int64_t* ep;
  const int32_t* push_step;
  float* push_rec;
  float settle_tol;
  // step response (ABI 10): cmd_rec NULL = none of these is read (pg, ep and settle_tol are shared)
  const int32_t* cmd_switch_step;
  float* cmd_rec;
  float yaw_tol;
  int steady_after;
};

extern "C++" {  // (templates and a struct return, inside the C ABI block)
// The prologue of the per-step record kernels (a group of lanes per env): whether the group's env
// exists, its record status and this step's reset flag, read by every lane of the group; tail lanes
// load nothing (status 1: frozen).
struct Recording { bool live; int st, rs; };
__device__ __forceinline__ Recording recording(const uint8_t* status, const uint8_t* reset, int e, int N) {
  const bool live = e < N;
  return {live, live ? status[e] : 1, live ? reset[e] : 0};
}
// A record row of Q float4 (16-byte accesses) <-> registers.
template <int Q>
__device__ __forceinline__ void load_row(const float4* p, float (&r)[4 * Q]) {
  LGX_UNROLL
  for (int i = 0; i < Q; ++i) {
    const float4 v = p[i];
    r[4 * i] = v.x; r[4 * i + 1] = v.y; r[4 * i + 2] = v.z; r[4 * i + 3] = v.w;
  }
}
template <int Q>
__device__ __forceinline__ void store_row(float4* p, const float (&r)[4 * Q]) {
  LGX_UNROLL
  for (int i = 0; i < Q; ++i) p[i] = make_float4(r[4 * i], r[4 * i + 1], r[4 * i + 2], r[4 * i + 3]);
}
}  // extern "C++"

// lgx_eval_accumulate: four lanes per env (16 envs per wave). Lane q of an env reads a quarter of
// the joints (consecutive lanes read consecutive addresses: 48 B of torques and 96 B of dof_state
// per env, whole lines per wave) and foot q; two xor shuffles combine the quarters; lane q then
// updates record columns 2q and 2q+1 (a wave writes 512 contiguous bytes). About 60 floats per
// env: the kernel is launch-bound. No LDS, no atomics; finished envs are read-only.
// Push recovery (push_rec set): lane q also updates push-record column q of a pushed env (a wave
// writes 256 contiguous bytes); the extra reads are the env's push_step, episode_length and
// projected_gravity rows.
// Step response (cmd_rec set): lane q also updates step-response columns 2q and 2q+1 of an env at
// or past its command switch (a wave writes 512 contiguous bytes); the extra reads are the env's
// cmd_switch_step, episode_length and projected_gravity rows.
__global__ __launch_bounds__(256) void eval_accumulate_kernel(EvalArgs A) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  const int e = t >> 2, q = t & 3;
  // no early return: the shuffles below need every lane of a group; tail lanes load nothing
  const auto [live, st, rs] = recording(A.status, A.reset, e, A.N);
  const bool sample = st == 0 && !rs;
  float en = 0.f, t2 = 0.f, fmax_ = 0.f;
  if (sample) {
    const int per = (A.D + 3) >> 2, j0 = q * per, j1 = min(A.D, j0 + per);
    const float* tq = A.torques + (size_t)e * A.D;
    const float* ds = A.dof_state + (size_t)e * A.D * 2;
    for (int j = j0; j < j1; ++j) {
      const float tau = tq[j], qd = ds[2 * j + 1];
      en += fabsf(tau * qd);
      t2 += tau * tau;
    }
    if (q < A.nfeet) {
      const float* c = A.contact + ((size_t)e * A.NB + A.feet[q]) * 3;
      fmax_ = sqrtf(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]);
    }
  }
  for (int o = 1; o <= 2; o <<= 1) {
    en += __shfl_xor(en, o, 64);
    t2 += __shfl_xor(t2, o, 64);
    fmax_ = fmaxf(fmax_, __shfl_xor(fmax_, o, 64));
  }
  if (!live || st != 0) return;
  if (rs) {
    if (q == 0) A.status[e] = episode_end_status(A.blew_up, A.time_out, e);
    return;
  }
  const float v0 = A.lin_vel[e * 3], v1 = A.lin_vel[e * 3 + 1], w2 = A.ang_vel[e * 3 + 2];
  const float c0 = A.commands[e * 4], c1 = A.commands[e * 4 + 1], c2 = A.commands[e * 4 + 2];
  float* a = A.acc + (size_t)e * LGX_EVAL_METRICS + 2 * q;
  float x0 = a[0], x1 = a[1];
  if (q == 0) {
    x0 += 1.0f;
    x1 += (c0 - v0) * (c0 - v0) + (c1 - v1) * (c1 - v1);
  } else if (q == 1) {
    x0 += (c2 - w2) * (c2 - w2);
    x1 += v0 * A.dt;
  } else if (q == 2) {
    x0 += sqrtf(v0 * v0 + v1 * v1) * A.dt;
    x1 += A.dt * en;
  } else {
    x0 += t2;
    x1 = fmaxf(x1, fmax_);
  }
  a[0] = x0;
  a[1] = x1;
  if (A.push_rec) {
    const int ps = A.push_step[e];
    const long long k = (long long)A.ep[e] - ps;
    if (ps > 0 && k > 0) {
      float* r = A.push_rec + (size_t)e * LGX_EVAL_PUSH_REC + q;
      *r = push_record_col(q, *r, A.pg + (size_t)e * 3, A.commands + (size_t)e * 4, A.lin_vel + (size_t)e * 3, k,
                           A.settle_tol);
    }
  }
  if (A.cmd_rec) {
    const int sw = A.cmd_switch_step[e];
    const long long k = (long long)A.ep[e] - sw;
    if (sw > 0 && k >= 0) {
      float* r = A.cmd_rec + (size_t)e * LGX_EVAL_CMD_REC + 2 * q;
      const float *pg = A.pg + (size_t)e * 3, *c = A.commands + (size_t)e * 4;
      const float *v = A.lin_vel + (size_t)e * 3, *w = A.ang_vel + (size_t)e * 3;
      const float y0 = command_record_col(2 * q, r[0], pg, c, v, w, k, A.settle_tol, A.yaw_tol, A.steady_after);
      const float y1 = command_record_col(2 * q + 1, r[1], pg, c, v, w, k, A.settle_tol, A.yaw_tol, A.steady_after);
      r[0] = y0;
      r[1] = y1;
    }
  }
}

// The reduce skeleton of lgx_eval_reduce / lgx_gait_reduce: THE definition of the tree (DESIGN.md
// "The reduce tree"; tests/test_gpu_reduce_tree.py pins it). One block of 256 threads per cell.
// Thread t scans envs t, t+256, ... in increasing order (the loads coalesce) and lets add(e, s) add
// what an env of this block's cell contributes to its NC fp64 partials s; the partials are combined
// by a fixed tree (shuffle-down inside each wave, then the four wave results in wave order), so the
// result depends only on the records. Every block scans every env's cell and so knows the number of
// out-of-grid envs, which is returned: when there are none, thread k < NC hands the sum of
// partial k to store(k, sum); when there are any, nothing is stored. (A caller that runs several
// passes puts a barrier between them: the previous pass's readers must be done with the exchange.)
extern "C++" {  // (a template, inside the C ABI block)
template <int NC, class Add, class Store>
__device__ __forceinline__ uint32_t cell_reduce(const int64_t* __restrict__ levels, const int64_t* __restrict__ types,
                                                const int32_t* __restrict__ cell_ids, int N, int rows, int cols,
                                                Add add, Store store) {
  __shared__ double part[4][NC];
  __shared__ uint32_t bad_s[4];
  const int cell = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  double s[NC];
  for (int k = 0; k < NC; ++k) s[k] = 0.0;
  uint32_t bad = 0;
  for (int e = tid; e < N; e += 256) {
    const int id = cell_of_env(levels, types, cell_ids, e, rows, cols);
    if (id < 0) { ++bad; continue; }
    if (id == cell) add(e, s);
  }
  for (int o = 32; o > 0; o >>= 1) {
    for (int k = 0; k < NC; ++k) s[k] += __shfl_down(s[k], o, 64);
    bad += __shfl_down(bad, o, 64);
  }
  if (lane == 0) {
    for (int k = 0; k < NC; ++k) part[wv][k] = s[k];
    bad_s[wv] = bad;
  }
  __syncthreads();
  const uint32_t nbad = bad_s[0] + bad_s[1] + bad_s[2] + bad_s[3];
  if (nbad == 0 && tid < NC) store(tid, ((part[0][tid] + part[1][tid]) + part[2][tid]) + part[3][tid]);
  return nbad;
}

// The maxima that ride a cell_reduce scan (lgx_joint_reduce, lgx_contact_reduce): every thread's NX
// fp32 partials x (a minimum as the maximum of the negated column, a "some env contributed" flag as
// the maximum of 0 / 1) are combined by fmaxf in cell_reduce's shape, shuffle-down inside each wave,
// then the four wave results, which folded(k) of the returned accessor forms for partial k after the
// barrier in here. A maximum does not depend on the order, so the result is exact. Called by every
// thread of the block, after cell_reduce (the caller's barrier between passes covers this exchange
// too).
template <int NX>
__device__ __forceinline__ auto cell_max(float (&x)[NX]) {
  __shared__ float xs[4][NX];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  for (int o = 32; o > 0; o >>= 1) {
    LGX_UNROLL
    for (int k = 0; k < NX; ++k) x[k] = fmaxf(x[k], __shfl_down(x[k], o, 64));
  }
  if (lane == 0) {
    LGX_UNROLL
    for (int k = 0; k < NX; ++k) xs[wv][k] = x[k];
  }
  __syncthreads();
  return [](int k) { return fmaxf(fmaxf(xs[0][k], xs[1][k]), fmaxf(xs[2][k], xs[3][k])); };
}
}  // extern "C++"

// lgx_eval_reduce: cell_reduce over the records of the cell's finished envs; block 0 publishes the
// out-of-grid count.
// ABI 9: cell_ids, when set, is the env's cell instead of level * cols + type (same range rule);
// push_cells, when set, gets the cell's push-recovery sums from push_rec by the same tree.
__global__ __launch_bounds__(256) void eval_reduce_kernel(const float* __restrict__ acc,
                                                          const uint8_t* __restrict__ status,
                                                          const int64_t* __restrict__ levels,
                                                          const int64_t* __restrict__ types,
                                                          const int32_t* __restrict__ cell_ids,
                                                          const float* __restrict__ push_rec, int N, int rows,
                                                          int cols, double* __restrict__ cells,
                                                          double* __restrict__ push_cells,
                                                          uint32_t* __restrict__ overflow) {
  constexpr int NA = LGX_EVAL_CELL_COLS, NC = NA + LGX_EVAL_PUSH_COLS;
  const int cell = blockIdx.x;
  const uint32_t nbad = cell_reduce<NC>(levels, types, cell_ids, N, rows, cols, [=](int e, auto& s) {
    const int st = status[e];
    s[0] += 1.0;
    if (st == 0) return;
    s[1] += st == 1 ? 1.0 : 0.0;  // time-out
    s[2] += st == 2 ? 1.0 : 0.0;  // fall
    s[3] += st == 3 ? 1.0 : 0.0;  // blow-up
    const float* a = acc + (size_t)e * LGX_EVAL_METRICS;
    for (int k = 0; k < LGX_EVAL_METRICS; ++k) s[4 + k] += (double)a[k];
    if (push_cells) {
      const float* r = push_rec + (size_t)e * LGX_EVAL_PUSH_REC;
      if (r[0] > 0.f) {
        s[NA + 0] += 1.0;
        s[NA + 1] += (double)r[1];
        s[NA + 2] += (double)r[2];
        s[NA + 3] += st == 1 ? 1.0 : 0.0;
        s[NA + 4] += st == 1 ? (double)r[3] : 0.0;
      }
    }
  }, [=](int k, double v) {
    if (k < NA) cells[(size_t)cell * NA + k] = v;
    else if (push_cells) push_cells[(size_t)cell * LGX_EVAL_PUSH_COLS + (k - NA)] = v;
  });
  if (threadIdx.x == 0 && cell == 0 && overflow) *overflow = nbad;
}

// lgx_eval_reduce's step-response cells (ABI 10, cmd_cells set): a second launch of the same
// shape as eval_reduce_kernel, cell_reduce over cmd_rec. It counts the out-of-grid envs itself, so
// it too writes nothing when there are any; eval_reduce_kernel publishes the count.
__global__ __launch_bounds__(256) void eval_cmd_reduce_kernel(const float* __restrict__ cmd_rec,
                                                              const uint8_t* __restrict__ status,
                                                              const int64_t* __restrict__ levels,
                                                              const int64_t* __restrict__ types,
                                                              const int32_t* __restrict__ cell_ids, int N, int rows,
                                                              int cols, double* __restrict__ cmd_cells) {
  constexpr int NC = LGX_EVAL_CMD_COLS;
  cell_reduce<NC>(levels, types, cell_ids, N, rows, cols, [=](int e, auto& s) {
    const int st = status[e];
    const float* r = cmd_rec + (size_t)e * LGX_EVAL_CMD_REC;
    if (st == 0 || !(r[0] > 0.f)) return;
    const bool surv = st == 1;
    s[0] += 1.0;
    s[1] += surv ? 1.0 : 0.0;
    s[2] += surv ? (double)r[1] : 0.0;
    s[3] += surv ? (double)r[2] : 0.0;
    s[4] += (double)r[3];
    for (int k = 4; k < LGX_EVAL_CMD_REC; ++k) s[1 + k] += surv ? (double)r[k] : 0.0;
  }, [=](int k, double v) { cmd_cells[(size_t)blockIdx.x * NC + k] = v; });
}
}  // namespace lgx

// The pieces the checks of the lgx_eval_* / lgx_trace_* / lgx_gait_* calls share. The common prefix:
// the env is bound and the call's buffers (kind: "eval", "trace", "gait") are given.
static int check_call(lgx_env* env, const void* bufs, const std::string& w, const char* kind) {
  if (!env) return -2;
  if (!env->bound) return fail(env, w + " before lgx_bind");
  if (!bufs) return fail(env, w + ": " + kind + " buffers are NULL");
  return 0;
}
// Every buffer of the table is bound; the failure is w + text + the first missing one's name.
struct NamedBuffer { const char* name; const void* ptr; };
static int check_bound(lgx_env* env, const std::string& w, const char* text,
                       std::initializer_list<NamedBuffer> table) {
  for (const NamedBuffer& t : table)
    if (!t.ptr) return fail(env, w + text + t.name);
  return 0;
}
static int check_feet(lgx_env* env, const std::string& w) {
  const lgx_task_params& p = env->params;
  for (int f = 0; f < p.num_feet; ++f)
    if (p.feet_idx[f] < 0 || p.feet_idx[f] >= p.num_bodies) return fail(env, w + ": feet_idx outside the bodies");
  return 0;
}
static const char* const kNotBound = ": required buffer not bound: ";

// The common prefix of the checks of the record families (lgx_gait_* / lgx_joint_* / lgx_contact_*):
// check_call, the family's record buffers in declaration order (NULL, then the alignment of those the
// kernels move as 16-byte accesses), status, overflow, cells (for the reduce) and the grid bound. The
// family goes on with its own scalars, bound buffers and params.
extern "C++" {  // (templates, inside the C ABI block)
template <class Bufs> struct RecordMember { const char* name; float* Bufs::*ptr; bool aligned; };
template <class Bufs>
static int record_buffers_check(lgx_env* env, const Bufs* b, const std::string& w, const char* kind,
                                std::initializer_list<RecordMember<Bufs>> records, bool reduce) {
  if (int rc = check_call(env, b, w, kind)) return rc;
  for (const RecordMember<Bufs>& r : records) {
    if (!(b->*r.ptr)) return fail(env, w + ": " + r.name + " is NULL");
    if (r.aligned && (uintptr_t)(b->*r.ptr) % 16 != 0) return fail(env, w + ": " + r.name + " must be 16-byte aligned");
  }
  if (!b->status) return fail(env, w + ": status is NULL");
  if (!b->overflow) return fail(env, w + ": overflow is NULL");
  if (reduce && !b->cells) return fail(env, w + ": cells is NULL");
  if (b->cell_rows < 1 || b->cell_cols < 1 || (int64_t)b->cell_rows * b->cell_cols > (1 << 20))
    return fail(env, w + ": cell_rows and cell_cols must be >= 1 (and their product at most 2^20)");
  return 0;
}
}  // extern "C++"
// The host backend's reduce found `bad` envs outside the cell grid.
static int reduce_failed(lgx_env* env, const char* name, int bad) {
  return fail(env, std::string(name) + ": " + std::to_string(bad) + " envs have a terrain level / type (or cell id) "
                   "outside the cell grid (cells not written)");
}
// Launch geometry, blocks of 256 threads: `lanes` threads per env; one block per cell.
static dim3 lane_blocks(int lanes, int N) { return dim3((unsigned)(((int64_t)lanes * N + 255) / 256)); }
static dim3 cell_blocks(int32_t rows, int32_t cols) { return dim3((unsigned)(rows * cols)); }

// shared checks of the three lgx_eval_* calls
static int eval_check(lgx_env* env, const lgx_eval_buffers* ev, const char* what, bool reduce) {
  const std::string w(what);
  if (int rc = check_call(env, ev, w, "eval")) return rc;
  const lgx_buffers& b = env->buffers;
  if (int rc = check_bound(env, w, kNotBound, {{"commands", b.commands}, {"base_lin_vel", b.base_lin_vel},
                                               {"base_ang_vel", b.base_ang_vel}, {"torques", b.torques},
                                               {"dof_state", b.dof_state}, {"contact_forces", b.contact_forces},
                                               {"reset", b.reset}, {"time_out", b.time_out}}))
    return rc;
  if (!ev->acc || !ev->status) return fail(env, w + ": acc and status are required");
  if (ev->cell_rows < 1 || ev->cell_cols < 1 || (int64_t)ev->cell_rows * ev->cell_cols > (1 << 20))
    return fail(env, w + ": cell_rows * cell_cols must be >= 1 (and at most 2^20)");
  if (reduce && (!ev->cells || !ev->overflow)) return fail(env, w + ": cells and overflow are required");
  if (ev->push_rec) {
    if (int rc = check_bound(env, w, ": push_rec needs a buffer that is not bound: ",
                             {{"projected_gravity", b.projected_gravity}, {"episode_length", b.episode_length},
                              {"push_step", b.push_step}, {"commands", b.commands}, {"base_lin_vel", b.base_lin_vel}}))
      return rc;
    if (!(ev->settle_tol >= 0.f)) return fail(env, w + ": settle_tol must be >= 0");
  }
  if (ev->push_cells && !ev->push_rec) return fail(env, w + ": push_cells needs push_rec");
  if (ev->cmd_rec) {
    if (!ev->cmd_switch_step) return fail(env, w + ": cmd_rec needs cmd_switch_step");
    if (int rc = check_bound(env, w, ": cmd_rec needs a buffer that is not bound: ",
                             {{"projected_gravity", b.projected_gravity}, {"episode_length", b.episode_length}}))
      return rc;
    if (!(ev->settle_tol >= 0.f)) return fail(env, w + ": settle_tol must be >= 0");
    if (!(ev->yaw_tol >= 0.f)) return fail(env, w + ": yaw_tol must be >= 0");
    if (ev->steady_after < 0) return fail(env, w + ": steady_after must be >= 0");
  }
  if (ev->cmd_cells && !ev->cmd_rec) return fail(env, w + ": cmd_cells needs cmd_rec");
  return check_feet(env, w);
}

int64_t lgx_sizeof_eval_buffers(void) { return (int64_t)sizeof(lgx_eval_buffers); }

int lgx_eval_begin(lgx_env* env, const lgx_eval_buffers* ev, void* hip_stream) {
  if (int rc = eval_check(env, ev, "lgx_eval_begin", false)) return rc;
  const size_t N = (size_t)env->params.num_envs;
  if (env->host) {
    lgxh::eval_begin(&env->params, ev);
    return 0;
  }
  hipStream_t st = (hipStream_t)hip_stream;
  HIP_OK(hipMemsetAsync(ev->acc, 0, sizeof(float) * LGX_EVAL_METRICS * N, st));
  HIP_OK(hipMemsetAsync(ev->status, 0, N, st));
  if (ev->overflow) HIP_OK(hipMemsetAsync(ev->overflow, 0, sizeof(uint32_t), st));
  if (ev->push_rec) HIP_OK(hipMemsetAsync(ev->push_rec, 0, sizeof(float) * LGX_EVAL_PUSH_REC * N, st));
  if (ev->cmd_rec) HIP_OK(hipMemsetAsync(ev->cmd_rec, 0, sizeof(float) * LGX_EVAL_CMD_REC * N, st));
  return 0;
}

int lgx_eval_accumulate(lgx_env* env, const lgx_eval_buffers* ev, void* hip_stream) {
  if (int rc = eval_check(env, ev, "lgx_eval_accumulate", false)) return rc;
  if (env->host) {
    lgxh::eval_accumulate(&env->params, &env->buffers, ev);
    return 0;
  }
  const lgx_buffers& b = env->buffers;
  const lgx_task_params& p = env->params;
  lgx::EvalArgs A;
  A.commands = b.commands; A.lin_vel = b.base_lin_vel; A.ang_vel = b.base_ang_vel; A.torques = b.torques;
  A.dof_state = b.dof_state; A.contact = b.contact_forces; A.reset = b.reset; A.time_out = b.time_out;
  A.blew_up = b.blew_up; A.acc = ev->acc; A.status = ev->status;
  A.pg = b.projected_gravity; A.ep = b.episode_length; A.push_step = b.push_step; A.push_rec = ev->push_rec;
  A.settle_tol = ev->settle_tol;
  A.cmd_switch_step = ev->cmd_switch_step; A.cmd_rec = ev->cmd_rec; A.yaw_tol = ev->yaw_tol;
  A.steady_after = ev->steady_after;
  A.N = p.num_envs; A.D = p.num_dof; A.NB = p.num_bodies; A.nfeet = p.num_feet; A.dt = p.dt;
  for (int f = 0; f < LGX_MAX_FEET; ++f) A.feet[f] = f < p.num_feet ? p.feet_idx[f] : 0;
  hipLaunchKernelGGL(lgx::eval_accumulate_kernel, lane_blocks(4, p.num_envs), dim3(256), 0, (hipStream_t)hip_stream, A);
  HIP_OK(hipGetLastError());
  return 0;
}

int lgx_eval_reduce(lgx_env* env, const lgx_eval_buffers* ev, void* hip_stream) {
  if (int rc = eval_check(env, ev, "lgx_eval_reduce", true)) return rc;
  if (env->host) {
    const int bad = lgxh::eval_reduce(&env->params, &env->buffers, ev);
    return bad ? reduce_failed(env, "lgx_eval_reduce", bad) : 0;
  }
  const lgx_buffers& b = env->buffers;
  hipLaunchKernelGGL(lgx::eval_reduce_kernel, cell_blocks(ev->cell_rows, ev->cell_cols), dim3(256), 0,
                     (hipStream_t)hip_stream, ev->acc, ev->status, b.terrain_levels, b.terrain_types, ev->cell_ids,
                     ev->push_rec, env->params.num_envs, ev->cell_rows, ev->cell_cols, ev->cells, ev->push_cells,
                     ev->overflow);
  HIP_OK(hipGetLastError());
  if (ev->cmd_cells) {
    hipLaunchKernelGGL(lgx::eval_cmd_reduce_kernel, cell_blocks(ev->cell_rows, ev->cell_cols), dim3(256), 0,
                       (hipStream_t)hip_stream, ev->cmd_rec, ev->status, b.terrain_levels, b.terrain_types,
                       ev->cell_ids, env->params.num_envs, ev->cell_rows, ev->cell_cols, ev->cmd_cells);
    HIP_OK(hipGetLastError());
  }
  return 0;
}

// ------------------------------------------------------------------ flight recorder (ABI 11)
namespace lgx {
// lgx_trace_record: sixteen lanes per env (4 envs per wave, a group never straddles a wave), five
// column passes: lane l writes columns l, l + 16, ..., so a pass stores 64 contiguous bytes per env
// and a row is 304 contiguous bytes. count[e], status[e] and reset[e] are read by every lane of the
// group before the first store of the kernel, and only lane 0 of the group writes count / status,
// after the row: no lane can see this launch's update (one thread per (env, column) spread over
// waves could). Lane l also forms the force norm of bodies l and l + 16; four xor shuffles fold the
// non-foot peak of columns 74 / 75 (trace_peak_merge is order-free). About 130 floats in and 76
// out per env (8.5 us at 4096 envs: latency, a twentieth of the HBM rate). No LDS, no atomics;
// frozen envs store nothing.
__global__ __launch_bounds__(256) void trace_record_kernel(const lgx_task_params* __restrict__ Pm,
                                                           const lgx_buffers* __restrict__ Bd, float* __restrict__ ring,
                                                           int32_t* __restrict__ count, uint8_t* __restrict__ status,
                                                           int depth) {
  const lgx_buffers& B = *Bd;
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  const int e = t >> 4, l = t & 15;
  // no early return: the shuffles below need every lane of a group; tail lanes load nothing
  const auto [live, st, rs] = recording(status, B.reset, e, Pm->num_envs);
  const int cnt = live ? count[e] : 0;
  const bool row = st == 0 && !rs;
  float pn = 0.f;
  int pb = -1;
  if (row) {
    const int NB = Pm->num_bodies;
    for (int b = l; b < NB; b += 16) {
      if (trace_is_foot(Pm, b)) continue;
      const float* c = B.contact_forces + ((size_t)e * NB + b) * 3;
      trace_peak_merge(pn, pb, nrm3(c[0], c[1], c[2]), b);
    }
  }
  for (int o = 1; o <= 8; o <<= 1) {
    const float on = __shfl_xor(pn, o, 64);
    const int ob = __shfl_xor(pb, o, 64);
    trace_peak_merge(pn, pb, on, ob);
  }
  if (!live || st != 0) return;
  if (rs) {
    if (l == 0) status[e] = episode_end_status(B, e);
    return;
  }
  float* dst = ring + ((size_t)e * depth + (size_t)(cnt % depth)) * LGX_TRACE_COLS;
  LGX_UNROLL
  for (int p = 0; p < 5; ++p) {
    const int col = l + 16 * p;
    if (col >= LGX_TRACE_COLS) break;
    dst[col] = col == 74 ? pn : (col == 75 ? (float)pb : trace_col(col, Pm, B, e));
  }
  if (l == 0) count[e] = cnt + 1;
}

// lgx_trace_gather: one thread per output float, grid-stride; consecutive lanes read consecutive
// addresses of a ring row and write consecutive addresses of the output (256 contiguous bytes per
// wave instruction on both sides). An id outside [0, N) is never used as an index.
__global__ __launch_bounds__(256) void trace_gather_kernel(const float* __restrict__ ring,
                                                           const int32_t* __restrict__ count,
                                                           const int32_t* __restrict__ ids, int N, int m, int depth,
                                                           float* __restrict__ out, int32_t* __restrict__ out_len) {
  const int64_t per = (int64_t)depth * LGX_TRACE_COLS, total = (int64_t)m * per;
  for (int64_t x = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; x < total; x += (int64_t)gridDim.x * blockDim.x) {
    const int i = (int)(x / per);
    const int64_t rem = x - (int64_t)i * per;
    const int r = (int)(rem / LGX_TRACE_COLS), c = (int)(rem % LGX_TRACE_COLS);
    const int e = ids[i];
    const bool ok = e >= 0 && e < N;
    const int cn = ok ? count[e] : 0;
    const int L = max(0, min(cn, depth));
    float v = 0.f;
    if (r >= depth - L) {
      const int slot = (cn - L + (r - (depth - L))) % depth;
      v = ring[((size_t)e * depth + slot) * LGX_TRACE_COLS + c];
    }
    out[x] = v;
    if (rem == 0) out_len[i] = ok ? L : -1;
  }
}
}  // namespace lgx

// shared checks of the three lgx_trace_* calls
static int trace_check(lgx_env* env, const lgx_trace_buffers* tb, const char* what, bool record) {
  const std::string w(what);
  if (int rc = check_call(env, tb, w, "trace")) return rc;
  if (tb->depth < 1) return fail(env, w + ": depth must be >= 1");
  if (!tb->ring) return fail(env, w + ": ring is NULL");
  if (!tb->count) return fail(env, w + ": count is NULL");
  if (!tb->status) return fail(env, w + ": status is NULL");
  if (!record) return 0;
  const lgx_buffers& b = env->buffers;
  if (int rc = check_bound(env, w, kNotBound,
                           {{"episode_length", b.episode_length}, {"root_states", b.root_states},
                            {"base_lin_vel", b.base_lin_vel}, {"base_ang_vel", b.base_ang_vel},
                            {"projected_gravity", b.projected_gravity}, {"commands", b.commands},
                            {"dof_state", b.dof_state}, {"torques", b.torques}, {"actions", b.actions},
                            {"contact_forces", b.contact_forces}, {"rew", b.rew}, {"reset", b.reset},
                            {"time_out", b.time_out}}))
    return rc;
  const lgx_task_params& p = env->params;
  if (p.num_dof > LGX_MAX_DOF || p.num_actions > LGX_MAX_DOF) return fail(env, w + ": more joints than a row holds");
  return check_feet(env, w);
}

int64_t lgx_sizeof_trace_buffers(void) { return (int64_t)sizeof(lgx_trace_buffers); }

int lgx_trace_begin(lgx_env* env, const lgx_trace_buffers* tb, void* hip_stream) {
  if (int rc = trace_check(env, tb, "lgx_trace_begin", false)) return rc;
  if (env->host) {
    lgxh::trace_begin(&env->params, tb);
    return 0;
  }
  const size_t N = (size_t)env->params.num_envs;
  hipStream_t st = (hipStream_t)hip_stream;
  HIP_OK(hipMemsetAsync(tb->ring, 0, sizeof(float) * LGX_TRACE_COLS * N * (size_t)tb->depth, st));
  HIP_OK(hipMemsetAsync(tb->count, 0, sizeof(int32_t) * N, st));
  HIP_OK(hipMemsetAsync(tb->status, 0, N, st));
  return 0;
}

int lgx_trace_record(lgx_env* env, const lgx_trace_buffers* tb, void* hip_stream) {
  if (int rc = trace_check(env, tb, "lgx_trace_record", true)) return rc;
  if (env->host) {
    lgxh::trace_record(&env->params, &env->buffers, tb);
    return 0;
  }
  hipLaunchKernelGGL(lgx::trace_record_kernel, lane_blocks(16, env->params.num_envs), dim3(256), 0,
                     (hipStream_t)hip_stream, env->d_params, env->d_buffers, tb->ring, tb->count, tb->status, tb->depth);
  HIP_OK(hipGetLastError());
  return 0;
}

int lgx_trace_gather(lgx_env* env, const lgx_trace_buffers* tb, const int32_t* ids, int32_t m, float* out,
                     int32_t* out_len, void* hip_stream) {
  if (int rc = trace_check(env, tb, "lgx_trace_gather", false)) return rc;
  if (m < 0) return fail(env, "lgx_trace_gather: m must be >= 0");
  if (m == 0) return 0;
  if (!ids) return fail(env, "lgx_trace_gather: ids is NULL");
  if (!out || !out_len) return fail(env, "lgx_trace_gather: out and out_len are required");
  if (env->host) {
    lgxh::trace_gather(&env->params, tb, ids, m, out, out_len);
    return 0;
  }
  const int64_t total = (int64_t)m * tb->depth * LGX_TRACE_COLS;
  const int64_t want = (total + 255) / 256, blocks = want < 2048 ? want : 2048;  // grid-stride beyond
  hipLaunchKernelGGL(lgx::trace_gather_kernel, dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)hip_stream, tb->ring,
                     tb->count, ids, env->params.num_envs, m, tb->depth, out, out_len);
  HIP_OK(hipGetLastError());
  return 0;
}

// ------------------------------------------------------------------ gait record (ABI 12)
namespace lgx {
// lgx_gait_record: four lanes per env (16 envs per wave, a group never straddles a wave), lane q =
// foot q. Each lane moves its foot's 16 record columns as four 16-byte accesses (64 contiguous
// bytes per lane, 4 KB per wave without gaps), keeps them in registers across gait_foot_sample, and
// reads its foot's contact force (12 B) and three floats of its rigid-body row. Two xor shuffles
// exchange the four contact bits; lane q then updates body columns 3q..3q+2 (48 contiguous bytes
// per env). status[e], reset[e] and body[e][0] (the "first sample" test) are read by every lane of
// the group before the first store of the kernel, and only lane 0 writes status and body[0]: no
// lane can see this launch's update. Per recording env: 256 + 48 B of records in and out, 4 x 24 B
// of sources and two flags in, about 700 B (5.0 us at 4096 envs: launch and load latency, a
// fourteenth of the HBM rate). No LDS, no atomics;
// frozen envs store nothing, tail lanes load nothing.
__global__ __launch_bounds__(256) void gait_record_kernel(const lgx_task_params* __restrict__ Pm,
                                                          const lgx_buffers* __restrict__ Bd, float* foot,
                                                          float* body, uint8_t* status) {
  const lgx_buffers& B = *Bd;
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  const int e = t >> 2, q = t & 3;
  // no early return: the shuffles below need every lane of a group
  const auto [live, st, rs] = recording(status, B.reset, e, Pm->num_envs);
  const bool sample = st == 0 && !rs;
  const int nfeet = Pm->num_feet;
  const bool mine = sample && q < nfeet;
  float* bq = body + (size_t)e * LGX_GAIT_BODY_COLS + 3 * q;
  float4* fq = reinterpret_cast<float4*>(foot + ((size_t)e * LGX_MAX_FEET + q) * LGX_GAIT_FOOT_COLS);
  float r[LGX_GAIT_FOOT_COLS], F[3] = {0.f, 0.f, 0.f}, R[13], b0 = 0.f, b1 = 0.f, b2 = 0.f;
  bool first = false;
  if (sample) {
    first = body[(size_t)e * LGX_GAIT_BODY_COLS] == 0.f;
    b0 = bq[0];
    b1 = bq[1];
    b2 = bq[2];
  }
  if (mine) {
    load_row<4>(fq, r);
    const size_t row = (size_t)e * Pm->num_bodies + Pm->feet_idx[q];
    const float* cf = B.contact_forces + row * 3;
    const float* rb = B.rigid_body_states + row * 13;
    F[0] = cf[0]; F[1] = cf[1]; F[2] = cf[2];
    R[2] = rb[2]; R[7] = rb[7]; R[8] = rb[8];
  }
  int bits = (mine && gait_contact(F)) ? (1 << q) : 0;
  bits |= __shfl_xor(bits, 1, 64);
  bits |= __shfl_xor(bits, 2, 64);
  if (!live || st != 0) return;
  if (rs) {
    if (q == 0) status[e] = episode_end_status(B, e);
    return;
  }
  if (mine) {
    gait_foot_sample(r, first, F, R, Pm->dt);
    store_row<4>(fq, r);
  }
  bq[0] = gait_body_col(3 * q, b0, bits, nfeet);
  bq[1] = gait_body_col(3 * q + 1, b1, bits, nfeet);
  bq[2] = gait_body_col(3 * q + 2, b2, bits, nfeet);
}

// lgx_gait_reduce: cell_reduce (above: the block shape, the env order and the tree) in five passes
// so that a thread holds at most 13 fp64 partials: pass 0 the 12 body columns, pass 1 + f foot f's
// columns 4..15, each in partials 0..11, and the env count in partial 12 (one layout for every pass
// keeps the partials in registers). Every pass scans every env's cell id in the same order, so
// the result depends only on the records (and every pass forms the same out-of-grid count): no
// block writes its cell when there are any, and block 0 publishes the count.
__global__ __launch_bounds__(256) void gait_reduce_kernel(const float* __restrict__ foot,
                                                          const float* __restrict__ body,
                                                          const uint8_t* __restrict__ status,
                                                          const int64_t* __restrict__ levels,
                                                          const int64_t* __restrict__ types,
                                                          const int32_t* __restrict__ cell_ids, int N, int rows,
                                                          int cols, double* __restrict__ cells,
                                                          uint32_t* __restrict__ overflow) {
  constexpr int NP = 1 + LGX_GAIT_BODY_COLS, NF = LGX_GAIT_FOOT_COLS - 4;
  static_assert(NF == LGX_GAIT_BODY_COLS, "a pass sums 12 columns (partials 0..11) and the env count (partial 12)");
  double* c = cells + (size_t)blockIdx.x * LGX_GAIT_CELL_COLS;
  for (int pass = 0; pass < 1 + LGX_MAX_FEET; ++pass) {
    if (pass) __syncthreads();  // the previous pass's readers are done with the exchange
    const uint32_t nbad = cell_reduce<NP>(levels, types, cell_ids, N, rows, cols, [=](int e, auto& s) {
      const float* b = body + (size_t)e * LGX_GAIT_BODY_COLS;
      if (status[e] == 0 || !(b[0] > 0.f)) return;
      const float* r = pass == 0 ? b : foot + ((size_t)e * LGX_MAX_FEET + (pass - 1)) * LGX_GAIT_FOOT_COLS + 4;
      for (int k = 0; k < NF; ++k) s[k] += (double)r[k];
      s[NF] += 1.0;  // the env count (stored by pass 0)
    }, [=](int k, double v) {
      if (k < NF) c[pass == 0 ? 1 + k : NP + NF * (pass - 1) + k] = v;
      else if (pass == 0) c[0] = v;
    });
    if (pass == 0 && threadIdx.x == 0 && blockIdx.x == 0) *overflow = nbad;
    if (nbad != 0) return;  // (uniform over the block)
  }
}
}  // namespace lgx

// shared checks of the three lgx_gait_* calls
static int gait_check(lgx_env* env, const lgx_gait_buffers* gb, const char* what, bool reduce) {
  const std::string w(what);
  if (int rc = record_buffers_check(env, gb, w, "gait", {{"foot", &lgx_gait_buffers::foot, true},
                                                         {"body", &lgx_gait_buffers::body, false}}, reduce))
    return rc;
  const lgx_buffers& b = env->buffers;
  if (int rc = check_bound(env, w, kNotBound, {{"contact_forces", b.contact_forces},
                                               {"rigid_body_states", b.rigid_body_states}, {"reset", b.reset},
                                               {"time_out", b.time_out}}))
    return rc;
  const int nf = env->params.num_feet;
  if (nf < 0 || nf > LGX_MAX_FEET) return fail(env, w + ": more feet than a record holds");
  return check_feet(env, w);
}

int64_t lgx_sizeof_gait_buffers(void) { return (int64_t)sizeof(lgx_gait_buffers); }

int lgx_gait_begin(lgx_env* env, const lgx_gait_buffers* gb, void* hip_stream) {
  if (int rc = gait_check(env, gb, "lgx_gait_begin", false)) return rc;
  if (env->host) {
    lgxh::gait_begin(&env->params, gb);
    return 0;
  }
  const size_t N = (size_t)env->params.num_envs;
  hipStream_t st = (hipStream_t)hip_stream;
  HIP_OK(hipMemsetAsync(gb->foot, 0, sizeof(float) * LGX_GAIT_FOOT_COLS * LGX_MAX_FEET * N, st));
  HIP_OK(hipMemsetAsync(gb->body, 0, sizeof(float) * LGX_GAIT_BODY_COLS * N, st));
  HIP_OK(hipMemsetAsync(gb->status, 0, N, st));
  HIP_OK(hipMemsetAsync(gb->overflow, 0, sizeof(uint32_t), st));
  return 0;
}

int lgx_gait_record(lgx_env* env, const lgx_gait_buffers* gb, void* hip_stream) {
  if (int rc = gait_check(env, gb, "lgx_gait_record", false)) return rc;
  if (env->host) {
    lgxh::gait_record(&env->params, &env->buffers, gb);
    return 0;
  }
  hipLaunchKernelGGL(lgx::gait_record_kernel, lane_blocks(4, env->params.num_envs), dim3(256), 0,
                     (hipStream_t)hip_stream, env->d_params, env->d_buffers, gb->foot, gb->body, gb->status);
  HIP_OK(hipGetLastError());
  return 0;
}

int lgx_gait_reduce(lgx_env* env, const lgx_gait_buffers* gb, void* hip_stream) {
  if (int rc = gait_check(env, gb, "lgx_gait_reduce", true)) return rc;
  if (env->host) {
    const int bad = lgxh::gait_reduce(&env->params, &env->buffers, gb);
    return bad ? reduce_failed(env, "lgx_gait_reduce", bad) : 0;
  }
  const lgx_buffers& b = env->buffers;
  hipLaunchKernelGGL(lgx::gait_reduce_kernel, cell_blocks(gb->cell_rows, gb->cell_cols), dim3(256), 0,
                     (hipStream_t)hip_stream, gb->foot, gb->body, gb->status, b.terrain_levels, b.terrain_types,
                     gb->cell_ids, env->params.num_envs, gb->cell_rows, gb->cell_cols, gb->cells, gb->overflow);
  HIP_OK(hipGetLastError());
  return 0;
}

// ------------------------------------------------------------------ joint-load record (ABI 13)
namespace lgx {
// lgx_joint_record: sixteen lanes per env (4 envs per wave, a group never straddles a wave), lane
// q < num_dof = joint q; lanes from num_dof on (12..15 at least) idle on the joint part. Each joint
// lane moves its joint's 16 record columns as four 16-byte accesses (64 contiguous bytes per lane,
// the env's 768 bytes and the wave's 3 KB without gaps), keeps them in registers across
// joint_sample, and reads its torque (4 B), its dof_state pair (8 B), its action (4 B) and its five
// limits from the device copy of the params (192 B that every group shares: cache hits). The total
// power P is joint_power_sum's four xor shuffles inside the group (offsets 1, 2, 4, 8), and the
// two "any joint" flags ride the same four stages as an OR. status[e], reset[e] and body[e] (one
// float4; its column 0 is the "first sample" test) are read by every lane of the group before the
// first store of the kernel, and only lane 0 writes status and body: no lane can see this launch's
// update. Per recording env: 768 + 16 B of records in and out, 12 x 16 B of sources and two flags
// in, about 1.8 KB. No LDS, no atomics; frozen envs store nothing, tail lanes load nothing.
__global__ __launch_bounds__(256) void joint_record_kernel(const lgx_task_params* __restrict__ Pm,
                                                           const lgx_buffers* __restrict__ Bd, float* joint,
                                                           float* body, uint8_t* status) {
  const lgx_buffers& B = *Bd;
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  const int e = t >> 4, q = t & 15;
  // no early return: the shuffles below need every lane of a group
  const auto [live, st, rs] = recording(status, B.reset, e, Pm->num_envs);
  const bool sample = st == 0 && !rs;
  const int D = Pm->num_dof;
  const bool mine = sample && q < D;
  float4* bq = reinterpret_cast<float4*>(body + (size_t)e * LGX_JOINT_BODY_COLS);
  float4* jq = reinterpret_cast<float4*>(joint + ((size_t)e * LGX_MAX_DOF + q) * LGX_JOINT_COLS);
  float r[LGX_JOINT_COLS], b[LGX_JOINT_BODY_COLS] = {0.f, 0.f, 0.f, 0.f}, ap = 0.f;
  bool sat = false, out = false;
  if (sample) load_row<1>(bq, b);
  if (mine) {
    load_row<4>(jq, r);
    const size_t j = (size_t)e * D + q;
    const float a = q < Pm->num_actions ? B.actions[(size_t)e * Pm->num_actions + q] : 0.f;
    ap = joint_sample(r, b[0] == 0.f, B.torques[j], B.dof_state[2 * j], B.dof_state[2 * j + 1], a,
                      Pm->torque_limits[q], Pm->dof_vel_limits[q], Pm->dof_pos_limits[q][0], Pm->dof_pos_limits[q][1],
                      Pm->clip_actions, Pm->dt, sat, out);
  }
  int any = (sat ? 1 : 0) | (out ? 2 : 0);
  const float P = joint_power_sum(ap, [&](float s, int o) {
    any |= __shfl_xor(any, o, 64);
    return __shfl_xor(s, o, 64);
  });
  if (!live || st != 0) return;
  if (rs) {
    if (q == 0) status[e] = episode_end_status(B, e);
    return;
  }
  if (mine) store_row<4>(jq, r);
  if (q == 0) {
    joint_body_sample(b, P, any & 1, any & 2);
    store_row<1>(bq, b);
  }
}

// lgx_joint_reduce: cell_reduce (above: the block shape, the env order and the tree) in six passes
// of two joints, so that a thread holds 35 fp64 partials: pass p sums columns 1..15 of joints
// 2p and 2p+1 in partials 0..29, the four body columns in partials 30..33 and the env count in partial
// 34 (one layout for every pass keeps the partials in registers; pass 0 stores the body sums and the
// count; three joints a pass take 256 VGPRs and spill into AGPRs, two take 205 and spill nothing).
// The maxima and minima ride the same scan in 12 fp32 partials x (per joint the maxima of
// columns 3, 6, 7, of -column 10 and of column 11; the max of body 1; 1 when an env contributed),
// combined by cell_max (above: exact); a cell without an env gets zeros. Every pass scans every
// env's cell id in the same order, so the result depends only on the records (and every pass forms
// the same out-of-grid count): no block writes its cell when there are any, and block 0 publishes
// the count.
__global__ __launch_bounds__(256) void joint_reduce_kernel(const float* __restrict__ joint,
                                                           const float* __restrict__ body,
                                                           const uint8_t* __restrict__ status,
                                                           const int64_t* __restrict__ levels,
                                                           const int64_t* __restrict__ types,
                                                           const int32_t* __restrict__ cell_ids, int N, int rows,
                                                           int cols, double* __restrict__ cells,
                                                           uint32_t* __restrict__ overflow) {
  constexpr int JP = 2, NS = LGX_JOINT_COLS - 1, NB = LGX_JOINT_BODY_COLS, NC = NS * JP + NB + 1, NX = 5 * JP + 2;
  static_assert(LGX_MAX_DOF % JP == 0, "every pass reduces JP joints");
  static_assert(LGX_JOINT_CELL_COLS == 2 + NB + LGX_MAX_DOF * (NS + 5), "the cell layout of include/lgx.h");
  const int tid = threadIdx.x;
  double* c = cells + (size_t)blockIdx.x * LGX_JOINT_CELL_COLS;
  for (int pass = 0; pass < LGX_MAX_DOF / JP; ++pass) {
    if (pass) __syncthreads();  // the previous pass's readers are done with the exchanges
    float x[NX];
    LGX_UNROLL
    for (int k = 0; k < NX; ++k) x[k] = -INFINITY;
    const uint32_t nbad = cell_reduce<NC>(levels, types, cell_ids, N, rows, cols, [&](int e, auto& s) {
      const float4 b = *reinterpret_cast<const float4*>(body + (size_t)e * NB);
      if (status[e] == 0 || !(b.x > 0.f)) return;
      LGX_UNROLL
      for (int jj = 0; jj < JP; ++jj) {
        const float4* r4 = reinterpret_cast<const float4*>(joint + ((size_t)e * LGX_MAX_DOF + JP * pass + jj) * LGX_JOINT_COLS);
        float r[LGX_JOINT_COLS];
        load_row<4>(r4, r);
        LGX_UNROLL
        for (int k = 0; k < NS; ++k) s[NS * jj + k] += (double)r[1 + k];
        x[5 * jj] = fmaxf(x[5 * jj], r[3]);
        x[5 * jj + 1] = fmaxf(x[5 * jj + 1], r[6]);
        x[5 * jj + 2] = fmaxf(x[5 * jj + 2], r[7]);
        x[5 * jj + 3] = fmaxf(x[5 * jj + 3], -r[10]);
        x[5 * jj + 4] = fmaxf(x[5 * jj + 4], r[11]);
      }
      s[NS * JP] += (double)b.x;
      s[NS * JP + 1] += (double)b.y;
      s[NS * JP + 2] += (double)b.z;
      s[NS * JP + 3] += (double)b.w;
      s[NC - 1] += 1.0;  // the env count (stored by pass 0)
      x[5 * JP] = fmaxf(x[5 * JP], b.y);
      x[5 * JP + 1] = 1.0f;
    }, [=](int k, double v) {
      if (k < NS * JP) c[2 + NB + (NS + 5) * (JP * pass + k / NS) + k % NS] = v;
      else if (pass == 0) c[k == NC - 1 ? 0 : 1 + (k - NS * JP)] = v;
    });
    if (pass == 0 && tid == 0 && blockIdx.x == 0) *overflow = nbad;
    if (nbad != 0) return;  // (uniform over the block)
    const auto folded = cell_max<NX>(x);
    if (tid < NX - 1 && (tid < 5 * JP || pass == 0)) {
      const bool some = folded(NX - 1) > 0.f;
      const float m = folded(tid);
      const double v = !some ? 0.0 : (double)(tid % 5 == 3 && tid < 5 * JP ? -m : m);
      if (tid < 5 * JP) c[2 + NB + (NS + 5) * (JP * pass + tid / 5) + NS + tid % 5] = v;
      else c[1 + NB] = v;
    }
  }
}
}  // namespace lgx

// shared checks of the three lgx_joint_* calls
static int joint_check(lgx_env* env, const lgx_joint_buffers* jb, const char* what, bool reduce) {
  const std::string w(what);
  if (int rc = record_buffers_check(env, jb, w, "joint", {{"joint", &lgx_joint_buffers::joint, true},
                                                          {"body", &lgx_joint_buffers::body, true}}, reduce))
    return rc;
  const lgx_buffers& b = env->buffers;
  if (int rc = check_bound(env, w, kNotBound, {{"torques", b.torques}, {"dof_state", b.dof_state},
                                               {"actions", b.actions}, {"reset", b.reset},
                                               {"time_out", b.time_out}}))
    return rc;
  const int nd = env->params.num_dof;
  if (nd < 0 || nd > LGX_MAX_DOF) return fail(env, w + ": more joints than a record holds");
  return 0;
}

int64_t lgx_sizeof_joint_buffers(void) { return (int64_t)sizeof(lgx_joint_buffers); }

int lgx_joint_begin(lgx_env* env, const lgx_joint_buffers* jb, void* hip_stream) {
  if (int rc = joint_check(env, jb, "lgx_joint_begin", false)) return rc;
  if (env->host) {
    lgxh::joint_begin(&env->params, jb);
    return 0;
  }
  const size_t N = (size_t)env->params.num_envs;
  hipStream_t st = (hipStream_t)hip_stream;
  HIP_OK(hipMemsetAsync(jb->joint, 0, sizeof(float) * LGX_JOINT_COLS * LGX_MAX_DOF * N, st));
  HIP_OK(hipMemsetAsync(jb->body, 0, sizeof(float) * LGX_JOINT_BODY_COLS * N, st));
  HIP_OK(hipMemsetAsync(jb->status, 0, N, st));
  HIP_OK(hipMemsetAsync(jb->overflow, 0, sizeof(uint32_t), st));
  return 0;
}

int lgx_joint_record(lgx_env* env, const lgx_joint_buffers* jb, void* hip_stream) {
  if (int rc = joint_check(env, jb, "lgx_joint_record", false)) return rc;
  if (env->host) {
    lgxh::joint_record(&env->params, &env->buffers, jb);
    return 0;
  }
  hipLaunchKernelGGL(lgx::joint_record_kernel, lane_blocks(16, env->params.num_envs), dim3(256), 0,
                     (hipStream_t)hip_stream, env->d_params, env->d_buffers, jb->joint, jb->body, jb->status);
  HIP_OK(hipGetLastError());
  return 0;
}

int lgx_joint_reduce(lgx_env* env, const lgx_joint_buffers* jb, void* hip_stream) {
  if (int rc = joint_check(env, jb, "lgx_joint_reduce", true)) return rc;
  if (env->host) {
    const int bad = lgxh::joint_reduce(&env->params, &env->buffers, jb);
    return bad ? reduce_failed(env, "lgx_joint_reduce", bad) : 0;
  }
  const lgx_buffers& b = env->buffers;
  hipLaunchKernelGGL(lgx::joint_reduce_kernel, cell_blocks(jb->cell_rows, jb->cell_cols), dim3(256), 0,
                     (hipStream_t)hip_stream, jb->joint, jb->body, jb->status, b.terrain_levels, b.terrain_types,
                     jb->cell_ids, env->params.num_envs, jb->cell_rows, jb->cell_cols, jb->cells, jb->overflow);
  HIP_OK(hipGetLastError());
  return 0;
}

// ------------------------------------------------------------------ contact record (ABI 14)
namespace lgx {
// lgx_contact_begin: body, status and overflow zero, every env row 0, 0, 0, 0, -1, 0, -1, 0 (the
// terminal columns' "none"), in one grid-stride launch of 16-byte stores.
__global__ __launch_bounds__(256) void contact_begin_kernel(float4* __restrict__ body, float4* __restrict__ envq,
                                                            uint8_t* __restrict__ status,
                                                            uint32_t* __restrict__ overflow, int N) {
  const size_t t = (size_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (size_t)gridDim.x * blockDim.x;
  const size_t nb = (size_t)N * (LGX_MAX_BODIES * LGX_CONTACT_COLS / 4), ne = (size_t)N * (LGX_CONTACT_ENV_COLS / 4);
  for (size_t i = t; i < nb; i += stride) body[i] = make_float4(0.f, 0.f, 0.f, 0.f);
  for (size_t i = t; i < ne; i += stride)
    envq[i] = (i & 1) ? make_float4(-1.f, 0.f, -1.f, 0.f) : make_float4(0.f, 0.f, 0.f, 0.f);
  for (size_t i = t; i < (size_t)N; i += stride) status[i] = 0;
  if (t == 0) *overflow = 0;
}

// lgx_contact_record: 32 lanes per env (2 envs per wave, a group never straddles a wave), lane
// q < num_bodies = body q; lanes from num_bodies on (24..31 at least) idle on the body part. Each
// body lane moves its body's 12 record columns as three 16-byte accesses (48 contiguous bytes per
// lane, the env's 1152 bytes without gaps), keeps them in registers across contact_body_sample, and
// reads its force (12 B), its position (12 B) and three int16 terrain samples, nine more only at a
// contact onset. The per-env part (contact_part: two counts and the two "largest fn, lowest index"
// arg-maxima) is combined by five xor shuffles inside the group (offsets 1..16); contact_merge is a
// total order and integer sums, so every lane ends with the same bits whatever the order. A group
// whose env is reset in this step (and still recording) loads its forces too: the terminal columns
// come from the same butterfly. status[e], reset[e] and env[e]'s first float4 (its column 0 is the
// "first sample" test) are read by every lane of the group before the first store of the kernel,
// and only lane 0 writes status and env (a sample: the first float4; a fall: the second): no lane
// can see this launch's update. No early return before the shuffles. Per recording env: 1152 + 16 B
// of records in and out, 24 x 24 B of sources, up to 24 x 3 (+ 9 at an onset) terrain samples and two
// flags, about 2.4 KB. No LDS, no atomics; frozen envs store nothing, tail lanes load nothing.
__global__ __launch_bounds__(256) void contact_record_kernel(const lgx_task_params* __restrict__ Pm,
                                                             const lgx_buffers* __restrict__ Bd, float* body,
                                                             float* envr, uint8_t* status, float edge_tol) {
  const lgx_buffers& B = *Bd;
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  const int e = t >> 5, q = t & 31;
  // no early return: the shuffles below need every lane of a group
  const auto [live, st, rs] = recording(status, B.reset, e, Pm->num_envs);
  const bool open = st == 0, sample = open && !rs;
  const int NB = Pm->num_bodies;
  const bool mine = open && q < NB;
  float4* eq = reinterpret_cast<float4*>(envr + (size_t)e * LGX_CONTACT_ENV_COLS);
  float4* bq = reinterpret_cast<float4*>(body + ((size_t)e * LGX_MAX_BODIES + q) * LGX_CONTACT_COLS);
  float r[LGX_CONTACT_COLS], v[4] = {0.f, 0.f, 0.f, 0.f};
  if (sample) load_row<1>(eq, v);
  contact_part p = contact_none();
  if (mine) {
    const size_t row = (size_t)e * NB + q;
    const float* F = B.contact_forces + row * 3;
    float fn;
    if (sample) {
      load_row<3>(bq, r);
      const int16_t* hs = Pm->mesh_type == LGX_MESH_PLANE ? nullptr : B.height_samples;
      fn = contact_body_sample(r, v[0] == 0.f, F, B.rigid_body_states + row * 13, Pm, hs, edge_tol);
    } else {
      fn = nrm3(F[0], F[1], F[2]);  // the step that ended the episode: the terminal columns
    }
    p = contact_body_part(Pm, q, fn);
  }
  LGX_UNROLL
  for (int o = 1; o < 32; o <<= 1) {
    contact_part other;
    other.pen = __shfl_xor(p.pen, o, 64);
    other.term = __shfl_xor(p.term, o, 64);
    other.tb = __shfl_xor(p.tb, o, 64);
    other.nb = __shfl_xor(p.nb, o, 64);
    other.tn = __shfl_xor(p.tn, o, 64);
    other.nn = __shfl_xor(p.nn, o, 64);
    contact_merge(p, other);
  }
  if (!live || !open) return;
  if (rs) {
    if (q == 0) {
      const int ns = episode_end_status(B, e);
      status[e] = (uint8_t)ns;
      if (ns == 2) {
        float w[4];
        contact_env_terminal(w, p);
        store_row<1>(eq + 1, w);
      }
    }
    return;
  }
  if (mine) store_row<3>(bq, r);
  if (q == 0) {
    contact_env_sample(v, p);
    store_row<1>(eq, v);
  }
}

// lgx_contact_reduce: cell_reduce (above: the block shape, the env order and the tree) in passes of
// BP bodies. A body has 10 sums (body columns 1, 2, 3, 5, 6, 8, 9, 11 and the two fall histograms,
// sums of (env column 4 == b) and (env column 6 == b) over the fallen, in the same scan), the env
// part 7 (the count, env columns 0..2, the fallen, the fallen without a termination contact, env
// column 7 over the fallen): a thread holds 10 BP + 7 fp64 partials, in one layout for every pass so
// that they stay in registers; pass 0 stores the env part. joint_reduce_kernel's reasoning fixes BP:
// there 35 partials fit (205 VGPRs, no spill) and 49 did not (256 VGPRs, spilling into AGPRs); three
// bodies a pass would be 37 partials, at that edge, so BP = 2 (27 partials; VGPR count in DESIGN.md).
// The maxima and minima ride the same scan in fp32 partials x (per body the maxima of columns 4, 10
// and of -column 7, the last over the envs with samples only; the max of env column 3; 1 when an env
// / an env with samples contributed), combined by cell_max (above: exact); a cell without a
// contributing env gets zeros. Every pass scans every env's cell id in
// the same order and forms the same out-of-grid count: no block writes its cell when there are any,
// and block 0 publishes the count.
__global__ __launch_bounds__(256) void contact_reduce_kernel(const float* __restrict__ body,
                                                             const float* __restrict__ envr,
                                                             const uint8_t* __restrict__ status,
                                                             const int64_t* __restrict__ levels,
                                                             const int64_t* __restrict__ types,
                                                             const int32_t* __restrict__ cell_ids, int N, int rows,
                                                             int cols, double* __restrict__ cells,
                                                             uint32_t* __restrict__ overflow) {
  constexpr int BP = 2, NS = 10, NE = 7, PER = 13, NC = NS * BP + NE, NX = 3 * BP + 3;
  static_assert(LGX_MAX_BODIES % BP == 0, "every pass reduces BP bodies");
  static_assert(LGX_CONTACT_CELL_COLS == 8 + LGX_MAX_BODIES * PER, "the cell layout of include/lgx.h");
  static_assert(LGX_CONTACT_COLS == 12 && LGX_CONTACT_ENV_COLS == 8, "three and two float4");
  const int tid = threadIdx.x;
  double* c = cells + (size_t)blockIdx.x * LGX_CONTACT_CELL_COLS;
  for (int pass = 0; pass < LGX_MAX_BODIES / BP; ++pass) {
    if (pass) __syncthreads();  // the previous pass's readers are done with the exchanges
    float x[NX];
    LGX_UNROLL
    for (int k = 0; k < NX; ++k) x[k] = -INFINITY;
    const uint32_t nbad = cell_reduce<NC>(levels, types, cell_ids, N, rows, cols, [&](int e, auto& s) {
      const int st = status[e];
      if (st == 0) return;
      const float4 e0 = *reinterpret_cast<const float4*>(envr + (size_t)e * LGX_CONTACT_ENV_COLS);
      const float4 e1 = *reinterpret_cast<const float4*>(envr + (size_t)e * LGX_CONTACT_ENV_COLS + 4);
      const bool fell = st == 2, sampled = e0.x > 0.f;
      LGX_UNROLL
      for (int jj = 0; jj < BP; ++jj) {
        const int b = BP * pass + jj;
        const float4* r4 = reinterpret_cast<const float4*>(body + ((size_t)e * LGX_MAX_BODIES + b) * LGX_CONTACT_COLS);
        const float4 r0 = r4[0], r1 = r4[1], r2 = r4[2];
        s[NS * jj] += (double)r0.y;       // column 1
        s[NS * jj + 1] += (double)r0.z;   // 2
        s[NS * jj + 2] += (double)r0.w;   // 3
        s[NS * jj + 3] += (double)r1.y;   // 5
        s[NS * jj + 4] += (double)r1.z;   // 6
        s[NS * jj + 5] += (double)r2.x;   // 8
        s[NS * jj + 6] += (double)r2.y;   // 9
        s[NS * jj + 7] += (double)r2.w;   // 11
        s[NS * jj + 8] += fell && e1.x == (float)b ? 1.0 : 0.0;
        s[NS * jj + 9] += fell && e1.z == (float)b ? 1.0 : 0.0;
        x[3 * jj] = fmaxf(x[3 * jj], r1.x);          // column 4
        x[3 * jj + 1] = fmaxf(x[3 * jj + 1], r2.z);  // column 10
        if (sampled) x[3 * jj + 2] = fmaxf(x[3 * jj + 2], -r1.w);  // column 7
      }
      s[NS * BP] += 1.0;
      s[NS * BP + 1] += (double)e0.x;
      s[NS * BP + 2] += (double)e0.y;
      s[NS * BP + 3] += (double)e0.z;
      s[NS * BP + 4] += fell ? 1.0 : 0.0;
      s[NS * BP + 5] += fell && e1.x < 0.f ? 1.0 : 0.0;
      s[NS * BP + 6] += fell ? (double)e1.w : 0.0;
      x[3 * BP] = fmaxf(x[3 * BP], e0.w);
      x[3 * BP + 1] = 1.0f;
      if (sampled) x[3 * BP + 2] = 1.0f;
    }, [=](int k, double v) {
      if (k < NS * BP) {
        const int kk = k % NS;
        c[8 + PER * (BP * pass + k / NS) + (kk < 8 ? kk : kk + 3)] = v;
      } else if (pass == 0) {
        const int i = k - NS * BP;  // cells 0, 1, 2, 3, 5, 6, 7 (4 is the maximum below)
        c[i < 4 ? i : i + 1] = v;
      }
    });
    if (pass == 0 && tid == 0 && blockIdx.x == 0) *overflow = nbad;
    if (nbad != 0) return;  // (uniform over the block)
    const auto folded = cell_max<NX>(x);
    if (tid < 3 * BP || (tid == 3 * BP && pass == 0)) {
      const int flag = (tid < 3 * BP && tid % 3 == 2) ? NX - 1 : NX - 2;
      const bool some = folded(flag) > 0.f;
      const float m = folded(tid);
      const double v = !some ? 0.0 : (double)(flag == NX - 1 ? -m : m);
      if (tid < 3 * BP) c[8 + PER * (BP * pass + tid / 3) + 8 + tid % 3] = v;
      else c[4] = v;
    }
  }
}
}  // namespace lgx

// shared checks of the three lgx_contact_* calls
static int contact_check(lgx_env* env, const lgx_contact_buffers* cb, const char* what, bool reduce) {
  const std::string w(what);
  if (int rc = record_buffers_check(env, cb, w, "contact", {{"body", &lgx_contact_buffers::body, true},
                                                            {"env", &lgx_contact_buffers::env, true}}, reduce))
    return rc;
  if (!std::isfinite(cb->edge_tol) || cb->edge_tol < 0.f)
    return fail(env, w + ": edge_tol must be finite and not negative");
  const lgx_buffers& b = env->buffers;
  if (int rc = check_bound(env, w, kNotBound, {{"contact_forces", b.contact_forces},
                                               {"rigid_body_states", b.rigid_body_states},
                                               {"reset", b.reset}, {"time_out", b.time_out}}))
    return rc;
  const lgx_task_params& p = env->params;
  if (p.num_bodies < 0 || p.num_bodies > LGX_MAX_BODIES) return fail(env, w + ": num_bodies outside [0, LGX_MAX_BODIES]");
  if (int rc = check_feet(env, w)) return rc;
  if (p.n_termination < 0 || p.n_termination > LGX_MAX_TERMINATION)
    return fail(env, w + ": n_termination outside termination_idx");
  for (int i = 0; i < p.n_termination; ++i)
    if (p.termination_idx[i] < 0 || p.termination_idx[i] >= p.num_bodies)
      return fail(env, w + ": termination_idx outside the bodies");
  if (p.n_penalised < 0 || p.n_penalised > LGX_MAX_PENALISED)
    return fail(env, w + ": n_penalised outside penalised_idx");
  for (int i = 0; i < p.n_penalised; ++i)
    if (p.penalised_idx[i] < 0 || p.penalised_idx[i] >= p.num_bodies)
      return fail(env, w + ": penalised_idx outside the bodies");
  if (p.mesh_type != LGX_MESH_PLANE) {
    if (!b.height_samples) return fail(env, w + kNotBound + "height_samples (the mesh is not a plane)");
    if (p.hf_rows < 3 || p.hf_cols < 3) return fail(env, w + ": hf_rows and hf_cols must be >= 3");
  }
  return 0;
}

int64_t lgx_sizeof_contact_buffers(void) { return (int64_t)sizeof(lgx_contact_buffers); }

int lgx_contact_begin(lgx_env* env, const lgx_contact_buffers* cb, void* hip_stream) {
  if (int rc = contact_check(env, cb, "lgx_contact_begin", false)) return rc;
  if (env->host) {
    lgxh::contact_begin(&env->params, cb);
    return 0;
  }
  const int N = env->params.num_envs;
  const int64_t quads = (int64_t)N * (LGX_MAX_BODIES * LGX_CONTACT_COLS / 4);
  const unsigned blocks = (unsigned)std::min<int64_t>(std::max<int64_t>((quads + 255) / 256, 1), 2048);
  hipLaunchKernelGGL(lgx::contact_begin_kernel, dim3(blocks), dim3(256), 0, (hipStream_t)hip_stream,
                     reinterpret_cast<float4*>(cb->body), reinterpret_cast<float4*>(cb->env), cb->status, cb->overflow, N);
  HIP_OK(hipGetLastError());
  return 0;
}

int lgx_contact_record(lgx_env* env, const lgx_contact_buffers* cb, void* hip_stream) {
  if (int rc = contact_check(env, cb, "lgx_contact_record", false)) return rc;
  if (env->host) {
    lgxh::contact_record(&env->params, &env->buffers, cb);
    return 0;
  }
  if (env->params.num_envs == 0) return 0;
  hipLaunchKernelGGL(lgx::contact_record_kernel, lane_blocks(32, env->params.num_envs), dim3(256), 0,
                     (hipStream_t)hip_stream, env->d_params, env->d_buffers, cb->body, cb->env, cb->status,
                     cb->edge_tol);
  HIP_OK(hipGetLastError());
  return 0;
}

int lgx_contact_reduce(lgx_env* env, const lgx_contact_buffers* cb, void* hip_stream) {
  if (int rc = contact_check(env, cb, "lgx_contact_reduce", true)) return rc;
  if (env->host) {
    const int bad = lgxh::contact_reduce(&env->params, &env->buffers, cb);
    return bad ? reduce_failed(env, "lgx_contact_reduce", bad) : 0;
  }
  const lgx_buffers& b = env->buffers;
  hipLaunchKernelGGL(lgx::contact_reduce_kernel, cell_blocks(cb->cell_rows, cb->cell_cols), dim3(256), 0,
                     (hipStream_t)hip_stream, cb->body, cb->env, cb->status, b.terrain_levels, b.terrain_types,
                     cb->cell_ids, env->params.num_envs, cb->cell_rows, cb->cell_cols, cb->cells, cb->overflow);
  HIP_OK(hipGetLastError());
  return 0;
}

#ifdef LGX_PHASE_CLOCK
// dev builds only: per-env phase cycle counters ([num_envs][16] uint32, device memory)
int lgx_debug_phase_buffer(uint32_t* dev_ptr) {
  return hipMemcpyToSymbol(HIP_SYMBOL(lgx::g_phase_out), &dev_ptr, sizeof(dev_ptr)) == hipSuccess ? 0 : -1;
}
#endif

const char* lgx_last_error(const lgx_env* env) { return env ? env->err.c_str() : "null env"; }

void lgx_destroy(lgx_env* env) {
  if (!env) return;
  if (env->host) {
    delete env;
    return;
  }
  if (env->d_model) (void)hipFree(env->d_model);
  if (env->d_params) (void)hipFree(env->d_params);
  if (env->d_buffers) (void)hipFree(env->d_buffers);
  delete env;
}

}  // extern "C"
