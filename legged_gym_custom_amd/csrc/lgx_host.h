// lgx_host.h — host (CPU) backend of include/lgx.h, selected by lgx_create(device < 0).
// Internal to liblgx.so: lgx_env.hip's C ABI dispatches here for host envs. Every buffer
// pointer in lgx_buffers is host memory; the stream arguments are ignored.
#pragma once
#include <stdint.h>

#include "../../include/lgx.h"

namespace lgxh {

// decimation x physics substeps (when `physics`) + post-physics for every env, OpenMP over
// envs; episode statistics of the envs that reset are summed in env order (deterministic).
void step(const lgx_model* M, const lgx_task_params* P, const lgx_buffers* B, uint64_t seed, uint64_t step,
          bool physics);
// reset_idx for the masked envs (RNG stream 1, counter = call)
void reset(const lgx_task_params* P, const lgx_buffers* B, const uint8_t* mask, uint64_t seed, uint64_t call);
// lgx_episode_extras on host buffers
void episode_extras(const lgx_task_params* P, const lgx_buffers* B, float* means, float* level_mean,
                    uint8_t* time_outs, uint64_t* step_counter);
// lgx_command_curriculum on host buffers
void command_curriculum(const lgx_task_params* P, const lgx_buffers* B, uint64_t seed, uint64_t step,
                        const double* global_sum_count);
// lgx_eval_begin on host buffers: zero the records (push_rec and cmd_rec too, when set) and the
// out-of-grid count
void eval_begin(const lgx_task_params* P, const lgx_eval_buffers* E);
// lgx_eval_accumulate on host buffers (OpenMP over envs; each env's joints summed in order; the
// push-recovery record of a pushed env when push_rec is set, the step-response record of an env at
// or past its command switch when cmd_rec is set)
void eval_accumulate(const lgx_task_params* P, const lgx_buffers* B, const lgx_eval_buffers* E);
// lgx_eval_reduce on host buffers, envs in order. Returns the number of envs whose level / type
// (or cell_ids entry) lies outside the cell grid; cells, push_cells and cmd_cells are written only
// when it is 0 (overflow always is).
int eval_reduce(const lgx_task_params* P, const lgx_buffers* B, const lgx_eval_buffers* E);
// lgx_trace_begin / lgx_trace_record / lgx_trace_gather on host buffers (OpenMP over envs, over
// the gathered ids): the flight recorder's rings, include/lgx.h ABI 11
void trace_begin(const lgx_task_params* P, const lgx_trace_buffers* T);
void trace_record(const lgx_task_params* P, const lgx_buffers* B, const lgx_trace_buffers* T);
void trace_gather(const lgx_task_params* P, const lgx_trace_buffers* T, const int32_t* ids, int32_t m, float* out,
                  int32_t* out_len);
// lgx_gait_begin / lgx_gait_record / lgx_gait_reduce on host buffers (OpenMP over envs; the
// reduction in env order): the gait record, include/lgx.h ABI 12. gait_reduce returns the number of
// envs outside the cell grid, as eval_reduce does.
void gait_begin(const lgx_task_params* P, const lgx_gait_buffers* G);
void gait_record(const lgx_task_params* P, const lgx_buffers* B, const lgx_gait_buffers* G);
int gait_reduce(const lgx_task_params* P, const lgx_buffers* B, const lgx_gait_buffers* G);
// lgx_joint_begin / lgx_joint_record / lgx_joint_reduce on host buffers (OpenMP over envs; the
// reduction in env order): the joint-load record, include/lgx.h ABI 13. joint_reduce returns the
// number of envs outside the cell grid, as eval_reduce does.
void joint_begin(const lgx_task_params* P, const lgx_joint_buffers* J);
void joint_record(const lgx_task_params* P, const lgx_buffers* B, const lgx_joint_buffers* J);
int joint_reduce(const lgx_task_params* P, const lgx_buffers* B, const lgx_joint_buffers* J);
// lgx_contact_begin / lgx_contact_record / lgx_contact_reduce on host buffers (OpenMP over envs; the
// reduction by the kernel's tree, so both backends give the same cells bit for bit): the contact
// record, include/lgx.h ABI 14. contact_reduce returns the number of envs outside the cell grid, as
// eval_reduce does.
void contact_begin(const lgx_task_params* P, const lgx_contact_buffers* C);
void contact_record(const lgx_task_params* P, const lgx_buffers* B, const lgx_contact_buffers* C);
int contact_reduce(const lgx_task_params* P, const lgx_buffers* B, const lgx_contact_buffers* C);
// the worker threads the host backend uses (OpenMP)
int threads();

}  // namespace lgxh
