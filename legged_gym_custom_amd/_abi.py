"""ctypes mirror of include/lgx.h (the C ABI of liblgx.so): the structs, the constants and the
function signatures, with the three tables _cbind.py describes at the end.

Field order and array sizes must match the header exactly: tests/test_abi.py compares every
field's offset and size, every constant and every parameter count with the compiled header, and a
loaded library (`_native.lib()`; the oracle through `check_layout()`) reports its own sizeof.
"""
import ctypes as C

ABI_VERSION = 17
MAX_DOF = 12
MAX_LINKS = 16
MAX_BODIES = 24
MAX_FEET = 4
MAX_PROPRIO = 240
MAX_HEIGHT_POINTS = 192
MAX_REWARDS = 40
MAX_CANDIDATES = 64
MAX_CONTACTS = 16
MAX_PENALISED = 24
MAX_TERMINATION = 8
EVAL_METRICS = 8     # per-env record columns (lgx_eval_buffers.acc)
EVAL_CELL_COLS = 12  # per-cell output columns (lgx_eval_buffers.cells)
MAX_ACTION_HISTORY = 4  # control steps of actuation latency (rows of lgx_buffers.action_history)
MAX_SENSOR_HISTORY = 4  # control steps of sensing latency (rows of lgx_buffers.sensor_history)
SCAN_STREAM = 3         # Philox stream of the height-scan model
EVAL_PUSH_REC = 4    # per-env push-recovery record columns (lgx_eval_buffers.push_rec)
EVAL_PUSH_COLS = 5   # per-cell push-recovery columns (lgx_eval_buffers.push_cells)
CMD_SEGMENTS = 4     # segments of an env's command schedule (lgx_buffers.cmd_step / cmd_val)
EVAL_CMD_REC = 8     # per-env step-response record columns (lgx_eval_buffers.cmd_rec)
EVAL_CMD_COLS = 9    # per-cell step-response columns (lgx_eval_buffers.cmd_cells)
TRACE_COLS = 76      # columns of a flight-recorder row (lgx_trace_buffers.ring)
GAIT_FOOT_COLS = 16  # per-env per-foot gait record columns (lgx_gait_buffers.foot)
GAIT_BODY_COLS = 12  # per-env gait record columns (lgx_gait_buffers.body)
GAIT_CELL_COLS = 61  # per-cell gait columns: 1 + 12 + MAX_FEET * 12 (lgx_gait_buffers.cells)
JOINT_COLS = 16      # per-env per-joint record columns (lgx_joint_buffers.joint)
JOINT_BODY_COLS = 4  # per-env record columns (lgx_joint_buffers.body)
JOINT_CELL_COLS = 246  # per-cell joint columns: 6 + MAX_DOF * 20 (lgx_joint_buffers.cells)
CONTACT_COLS = 12      # per-env per-body record columns (lgx_contact_buffers.body)
CONTACT_ENV_COLS = 8   # per-env record columns (lgx_contact_buffers.env)
CONTACT_CELL_COLS = 320  # per-cell contact columns: 8 + MAX_BODIES * 13 (lgx_contact_buffers.cells)

TASK_LEGGED = 0
TASK_GO2 = 1
MESH_PLANE, MESH_HEIGHTFIELD, MESH_TRIMESH = 0, 1, 2
CONTROL = {"P": 0, "V": 1, "T": 2}

# enum lgx_reward_id (include/lgx.h) — name -> id
REWARD_IDS = {name: i for i, name in enumerate([
    "action_rate", "ang_vel_xy", "base_height", "calf_collision", "calf_pos", "calf_symmetry",
    "collision", "delta_torques", "dof_acc", "dof_error", "dof_pos_limits", "dof_vel",
    "dof_vel_limits", "feet_air_time", "feet_contact_forces", "heading_alignment", "hip_pos",
    "jump_zone_forward_vel", "jump_zone_upward_vel", "lin_vel_z", "min_height", "orientation",
    "phase_contact_match", "phase_foot_lifting", "reverse_penalty", "stand_still", "stumble_calves",
    "stumble_feet", "thigh_pos", "thigh_symmetry", "torque_limits", "torques", "tracking_ang_vel",
    "tracking_lin_vel", "tracking_pitch", "tracking_roll", "zero_cmd_dof_error",
])}

f32 = C.c_float
i32 = C.c_int32


class Model(C.Structure):
    _fields_ = [
        ("num_links", i32), ("num_bodies", i32), ("num_candidates", i32),
        ("link_parent", i32 * MAX_LINKS),
        ("joint_origin", (f32 * 3) * MAX_LINKS),
        ("joint_axis", (f32 * 3) * MAX_LINKS),
        ("joint_rot", (f32 * 9) * MAX_LINKS),
        ("joint_lower", f32 * MAX_LINKS),
        ("joint_upper", f32 * MAX_LINKS),
        ("joint_has_limits", i32 * MAX_LINKS),
        ("link_mass", f32 * MAX_LINKS),
        ("link_com", (f32 * 3) * MAX_LINKS),
        ("link_inertia", (f32 * 6) * MAX_LINKS),
        ("body_link", i32 * MAX_BODIES),
        ("body_offset", (f32 * 3) * MAX_BODIES),
        ("body_rot", (f32 * 9) * MAX_BODIES),
        ("cand_link", i32 * MAX_CANDIDATES),
        ("cand_body", i32 * MAX_CANDIDATES),
        ("cand_pos", (f32 * 3) * MAX_CANDIDATES),
        ("cand_radius", f32 * MAX_CANDIDATES),
    ]


class TaskParams(C.Structure):
    _fields_ = [
        ("abi_version", i32), ("task_kind", i32), ("num_envs", i32), ("num_envs_total", i32),
        ("env_id_offset", i32),
        ("num_dof", i32), ("num_bodies", i32), ("num_actions", i32), ("num_feet", i32),
        ("num_proprio", i32), ("history_len", i32), ("num_obs", i32), ("num_priv", i32), ("num_est", i32),
        ("num_scan", i32), ("num_critic", i32),
        ("num_height_points", i32), ("num_reward_terms", i32), ("decimation", i32),
        ("sim_dt", f32), ("dt", f32),
        ("action_scale", f32), ("clip_actions", f32), ("clip_obs", f32),
        ("control_type", i32), ("randomize_kp_kd", i32),
        ("p_gains", f32 * MAX_DOF), ("d_gains", f32 * MAX_DOF), ("default_dof_pos", f32 * MAX_DOF),
        ("torque_limits", f32 * MAX_DOF), ("dof_pos_limits", (f32 * 2) * MAX_DOF),
        ("dof_vel_limits", f32 * MAX_DOF),
        ("soft_dof_vel_limit", f32), ("soft_torque_limit", f32),
        ("obs_scale_lin_vel", f32), ("obs_scale_ang_vel", f32), ("obs_scale_dof_pos", f32),
        ("obs_scale_dof_vel", f32), ("obs_scale_height", f32),
        ("add_noise", i32), ("noise_vec", f32 * MAX_PROPRIO),
        ("measure_heights", i32), ("height_points", (f32 * 2) * MAX_HEIGHT_POINTS),
        ("heading_command", i32), ("zero_command", i32), ("resample_interval", i32), ("has_user_command", i32),
        ("cmd_lin_vel_x", f32 * 2), ("cmd_lin_vel_y", f32 * 2), ("cmd_ang_vel_yaw", f32 * 2),
        ("cmd_heading", f32 * 2),
        ("heading_error_gain", f32), ("zero_command_prob", f32),
        ("user_command", f32 * 4), ("commands_scale", f32 * 3),
        ("period", f32), ("offset_fl", f32), ("offset_fr", f32), ("offset_bl", f32), ("offset_br", f32),
        ("max_episode_length", i32), ("max_episode_length_s", f32), ("parkour", i32),
        ("n_termination", i32), ("termination_idx", i32 * MAX_TERMINATION),
        ("n_penalised", i32), ("penalised_idx", i32 * MAX_PENALISED),
        ("feet_idx", i32 * MAX_FEET), ("calf_idx", i32 * MAX_FEET),
        ("hip_joint_idx", i32 * MAX_FEET), ("thigh_joint_idx", i32 * MAX_FEET), ("calf_joint_idx", i32 * MAX_FEET),
        ("reward_ids", i32 * MAX_REWARDS), ("reward_scales", f32 * MAX_REWARDS),
        ("only_positive_rewards", i32), ("has_termination_reward", i32), ("termination_scale", f32),
        ("tracking_sigma", f32), ("base_height_target", f32), ("max_foot_height", f32),
        ("percent_time_on_ground", f32),
        ("max_contact_force", f32), ("pitch_deg_target", f32), ("roll_deg_target", f32),
        ("push_robots", i32), ("push_interval", i32), ("max_push_vel_xy", f32),
        ("base_init_state", f32 * 13), ("custom_origins", i32),
        ("mesh_type", i32), ("horizontal_scale", f32), ("vertical_scale", f32), ("border_size", f32),
        ("hf_rows", i32), ("hf_cols", i32),
        ("curriculum", i32), ("terrain_length", f32), ("promote_threshold", f32), ("demote_threshold", f32),
        ("max_terrain_level", i32), ("num_terrain_rows", i32), ("num_terrain_cols", i32),
        ("gravity", f32 * 3), ("ground_friction", f32), ("solver_iterations", i32),
        ("baumgarte", f32), ("slop", f32), ("max_depenetration_vel", f32), ("contact_margin", f32),
        ("limit_margin", f32),
        ("actuator_net", i32), ("sea_in_scale", f32 * 2), ("sea_out_scale", f32), ("sea_lin_b", f32),
        ("sea_w_ih0", f32 * 64), ("sea_w_hh0", f32 * 256), ("sea_b_ih0", f32 * 32), ("sea_b_hh0", f32 * 32),
        ("sea_w_ih1", f32 * 256), ("sea_w_hh1", f32 * 256), ("sea_b_ih1", f32 * 32), ("sea_b_hh1", f32 * 32),
        ("sea_lin_w", f32 * 8),
        ("command_curriculum", i32), ("curriculum_term", i32), ("curriculum_threshold", f32),
        ("curriculum_lo_free", i32), ("curriculum_delta", C.c_double), ("curriculum_lo_min", C.c_double),
        ("curriculum_lo_max", C.c_double), ("curriculum_hi_max", C.c_double),
        ("action_history_len", i32), ("sensor_history_len", i32),
    ]


P = C.c_void_p


class Buffers(C.Structure):
    _fields_ = [(name, P) for name in [
        "root_states", "dof_state", "contact_forces", "rigid_body_states",
        "actions_in", "actions", "torques",
        "last_actions", "last_dof_vel", "last_root_vel", "last_base_lin_vel", "last_torques",
        "commands", "episode_length", "episode_sums", "obs_history", "last_contacts",
        "last_contact_heights", "feet_air_time",
        "obs", "priv", "critic", "est", "scan", "rew", "reset", "time_out",
        "base_lin_vel", "base_ang_vel", "projected_gravity", "rpy_phase", "measured_heights",
        "friction", "mass_params", "kp_kd", "env_origins", "terrain_levels", "terrain_types",
        "terrain_origins", "height_samples", "terrain_mesh", "sea_hidden", "sea_cell", "episode_stats",
        "blew_up", "blowup_count", "command_ranges", "curriculum_vals", "command_range_log",
        "action_delay", "action_history", "motor_strength", "push_step", "push_dvel", "cmd_step", "cmd_val",
        "obs_noise_scale", "obs_bias", "obs_delay", "sensor_history", "sensor_count",
        "force_window", "force_vec",
        "scan_noise", "scan_dropout", "scan_offset", "scan_delay", "scan_history",
    ]]


BUFFER_FIELDS = [f[0] for f in Buffers._fields_]


class EvalBuffers(C.Structure):
    """lgx_eval_buffers (ABI 7; cell_ids and the push-recovery members: ABI 9; the step-response
    members: ABI 10): the policy evaluation's records and cells."""
    _fields_ = [("acc", P), ("status", P), ("cells", P), ("overflow", P), ("cell_rows", i32), ("cell_cols", i32),
                ("cell_ids", P), ("push_rec", P), ("settle_tol", f32), ("push_cells", P),
                ("cmd_switch_step", P), ("cmd_rec", P), ("cmd_cells", P), ("yaw_tol", f32), ("steady_after", i32)]


class TraceBuffers(C.Structure):
    """lgx_trace_buffers (ABI 11): the flight recorder's per-env rings."""
    _fields_ = [("ring", P), ("count", P), ("status", P), ("depth", i32)]


class GaitBuffers(C.Structure):
    """lgx_gait_buffers (ABI 12): the gait record's per-env per-foot records and per-cell sums."""
    _fields_ = [("foot", P), ("body", P), ("status", P), ("cells", P), ("overflow", P), ("cell_rows", i32),
                ("cell_cols", i32), ("cell_ids", P)]


class JointBuffers(C.Structure):
    """lgx_joint_buffers (ABI 13): the joint-load record's per-env per-joint records and per-cell sums."""
    _fields_ = [("joint", P), ("body", P), ("status", P), ("cells", P), ("overflow", P), ("cell_rows", i32),
                ("cell_cols", i32), ("cell_ids", P)]


class ContactBuffers(C.Structure):
    """lgx_contact_buffers (ABI 14): the contact record's per-env per-body records and per-cell sums."""
    _fields_ = [("body", P), ("env", P), ("status", P), ("cells", P), ("overflow", P), ("cell_rows", i32),
                ("cell_cols", i32), ("cell_ids", P), ("edge_tol", f32)]


STRUCTS = {"lgx_model": Model, "lgx_task_params": TaskParams, "lgx_buffers": Buffers,
           "lgx_eval_buffers": EvalBuffers, "lgx_trace_buffers": TraceBuffers, "lgx_gait_buffers": GaitBuffers,
           "lgx_joint_buffers": JointBuffers, "lgx_contact_buffers": ContactBuffers}
SIZEOF = {"lgx_sizeof_" + name[len("lgx_"):]: name for name in STRUCTS}  # sizeof export -> typedef

# The record families of the evaluation (lgx_<kind>_begin / _record / _reduce): kind -> (the struct,
# its two record members with their per-env shapes, the columns of a cell row, the extra scalar
# members). All share status, cells, overflow, cell_rows, cell_cols and cell_ids.
RECORD_KINDS = {
    "gait": (GaitBuffers, (("foot", (MAX_FEET, GAIT_FOOT_COLS)), ("body", (GAIT_BODY_COLS,))), GAIT_CELL_COLS, ()),
    "joint": (JointBuffers, (("joint", (MAX_DOF, JOINT_COLS)), ("body", (JOINT_BODY_COLS,))), JOINT_CELL_COLS, ()),
    "contact": (ContactBuffers, (("body", (MAX_BODIES, CONTACT_COLS)), ("env", (CONTACT_ENV_COLS,))), CONTACT_CELL_COLS,
                ("edge_tol",)),
}

CONSTANTS = {
    "LGX_ABI_VERSION": ABI_VERSION, "LGX_MAX_DOF": MAX_DOF, "LGX_MAX_LINKS": MAX_LINKS,
    "LGX_MAX_BODIES": MAX_BODIES, "LGX_MAX_FEET": MAX_FEET, "LGX_MAX_PROPRIO": MAX_PROPRIO,
    "LGX_MAX_HEIGHT_POINTS": MAX_HEIGHT_POINTS, "LGX_MAX_REWARDS": MAX_REWARDS,
    "LGX_MAX_CANDIDATES": MAX_CANDIDATES, "LGX_MAX_CONTACTS": MAX_CONTACTS, "LGX_MAX_PENALISED": MAX_PENALISED,
    "LGX_MAX_TERMINATION": MAX_TERMINATION, "LGX_EVAL_METRICS": EVAL_METRICS, "LGX_EVAL_CELL_COLS": EVAL_CELL_COLS,
    "LGX_MAX_ACTION_HISTORY": MAX_ACTION_HISTORY, "LGX_MAX_SENSOR_HISTORY": MAX_SENSOR_HISTORY, "LGX_SCAN_STREAM": SCAN_STREAM,
    "LGX_EVAL_PUSH_REC": EVAL_PUSH_REC, "LGX_EVAL_PUSH_COLS": EVAL_PUSH_COLS,
    "LGX_CMD_SEGMENTS": CMD_SEGMENTS, "LGX_EVAL_CMD_REC": EVAL_CMD_REC, "LGX_EVAL_CMD_COLS": EVAL_CMD_COLS,
    "LGX_TRACE_COLS": TRACE_COLS,
    "LGX_GAIT_FOOT_COLS": GAIT_FOOT_COLS, "LGX_GAIT_BODY_COLS": GAIT_BODY_COLS, "LGX_GAIT_CELL_COLS": GAIT_CELL_COLS,
    "LGX_JOINT_COLS": JOINT_COLS, "LGX_JOINT_BODY_COLS": JOINT_BODY_COLS, "LGX_JOINT_CELL_COLS": JOINT_CELL_COLS,
    "LGX_CONTACT_COLS": CONTACT_COLS, "LGX_CONTACT_ENV_COLS": CONTACT_ENV_COLS,
    "LGX_CONTACT_CELL_COLS": CONTACT_CELL_COLS,
    "LGX_TASK_LEGGED": TASK_LEGGED, "LGX_TASK_GO2": TASK_GO2,
    "LGX_MESH_PLANE": MESH_PLANE, "LGX_MESH_HEIGHTFIELD": MESH_HEIGHTFIELD, "LGX_MESH_TRIMESH": MESH_TRIMESH,
    **{"LGX_CONTROL_" + name: v for name, v in CONTROL.items()},
    **{"LGX_REW_" + name.upper(): v for name, v in REWARD_IDS.items()},
    "LGX_REW_COUNT": len(REWARD_IDS),
}

u64, cint = C.c_uint64, C.c_int
SIGNATURES = {
    "lgx_abi_version": (i32, ()),
    **{name: (C.c_int64, ()) for name in SIZEOF},
    "lgx_create": (cint, (P, P, i32, C.POINTER(P))),
    "lgx_bind": (cint, (P, P)),
    "lgx_step": (cint, (P, u64, u64, P)),
    "lgx_step_dev": (cint, (P, u64, P, P)),
    "lgx_post_physics": (cint, (P, u64, u64, P)),
    "lgx_physics": (cint, (P, P)),
    "lgx_reset_envs": (cint, (P, P, u64, u64, P)),
    "lgx_episode_extras": (cint, (P, P, P, P, P, P)),
    "lgx_command_curriculum": (cint, (P, u64, u64, P, P, P)),
    "lgx_set_envs_per_wave": (cint, (P, i32)),
    "lgx_eval_begin": (cint, (P, P, P)),
    "lgx_eval_accumulate": (cint, (P, P, P)),
    "lgx_eval_reduce": (cint, (P, P, P)),
    "lgx_trace_begin": (cint, (P, P, P)),
    "lgx_trace_record": (cint, (P, P, P)),
    "lgx_trace_gather": (cint, (P, P, P, i32, P, P, P)),
    "lgx_gait_begin": (cint, (P, P, P)),
    "lgx_gait_record": (cint, (P, P, P)),
    "lgx_gait_reduce": (cint, (P, P, P)),
    "lgx_joint_begin": (cint, (P, P, P)),
    "lgx_joint_record": (cint, (P, P, P)),
    "lgx_joint_reduce": (cint, (P, P, P)),
    "lgx_contact_begin": (cint, (P, P, P)),
    "lgx_contact_record": (cint, (P, P, P)),
    "lgx_contact_reduce": (cint, (P, P, P)),
    "lgx_last_error": (C.c_char_p, (P,)),
    "lgx_destroy": (None, (P,)),
}


def check_layout(lib, prefix):
    """Compare ctypes sizes with the `<prefix><name>` sizeof exports a library has (the oracle's
    `oracle_sizeof_{model,params,buffers}`; liblgx.so's own are checked when `_native.lib()` loads it)."""
    for name, cls in (("model", Model), ("params", TaskParams), ("buffers", Buffers), ("eval_buffers", EvalBuffers)):
        try:
            fn = C.CFUNCTYPE(C.c_int64)((prefix + name, lib))
        except AttributeError:
            continue
        n = fn()
        if n != C.sizeof(cls):
            raise RuntimeError(f"ABI layout mismatch for {name}: native {n} vs ctypes {C.sizeof(cls)}")
