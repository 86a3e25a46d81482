"""Shared by tests/test_gpu_sensor.py (device "cuda:0") and tests/test_sensor_host.py (the same
bodies on the host backend): the per-env sensor model (include/lgx.h, ABI 15): observation-noise
level, constant bias and sensing latency.

The feature has no oracle. As tests/actuator_case.py does, every test reduces feature-on behaviour
to feature-off behaviour, which the oracle and the golden fixtures pin. Env X (feature) and env Y
(plain) are built with the same seed and fed the same scripted actions; the sensor model touches
observations only, so X's physics buffers equal Y's bit for bit at every step (asserted), and
  * a latency of d control steps is Y's current-observation row of d steps ago on the sensor
    channels (never across a reset), Y's row of this step elsewhere: bit-exact;
  * a bias is Y's row plus the bias in fp32: bit-exact;
  * a noise scale s is Z + s (Y - Z) with Z the env without noise: exact for s in {0, 1}, else within
    (1 + s) 2^-23 max(|X|, |Y|, |Z|), the fp32 rounding of the two sums and the product.
Resets happen inside every run: the episode is 20 steps long and the episode lengths are staggered
in place in both envs, so a third of the envs time out within the first steps.
Kernel against host backend: the bounds of tests/actuator_case.py (2e-3 + 1e-3 |ref|)."""
import math

import torch

from actuator_case import DISCRETE, PHYSICS, assert_equal, bound, copy_state, make_env, worst_ratio

K = 3  # control steps of sensor history in the latency tests
EPISODE_STEPS = 20
CASES = [("go2", 64, 12), ("go2", 63, 12), ("go2_parkour", 64, 10), ("anymal_c_rough", 64, 8)]


def capacity(k=K):
    """domain_rand.max_obs_delay_s for k control steps of sensor history."""
    return lambda cfg: k * cfg.control.decimation * cfg.sim.dt


def short_episode(cfg):
    return EPISODE_STEPS * cfg.control.decimation * cfg.sim.dt


def stagger(*envs):
    """After reset(): a third of the envs close to their time-out, the rest at 0, in place."""
    n = envs[0].num_envs
    last = int(envs[0].max_episode_length)
    e = torch.arange(n)
    lens = torch.where(e % 3 == 0, last - 1 - e % 4, torch.zeros_like(e))
    for env in envs:
        assert int(env.max_episode_length) == last
        env.episode_length_buf = lens.to(env.device)


def dims(env):
    P = env.task_params
    return int(P.history_len), int(P.num_proprio)


def cur_row(env, buf=None):
    """The current-observation row of obs (or of the Go2 critic's copy)."""
    H, Pp = dims(env)
    return (env.obs_buf if buf is None else buf)[:, H * Pp:H * Pp + Pp]


def sensor_mask(env):
    """[P] bool: the sensor channels, from the layout."""
    _, Pp = dims(env)
    m = torch.zeros(Pp, dtype=torch.bool)
    for name, sl in env.obs_channel_groups().items():
        if name not in ("command", "actions", "phase"):
            m[sl] = True
    return m


def same_physics(X, Y, what):
    bx, by = bound(X), bound(Y)
    assert_equal(bx, by, PHYSICS + tuple(k for k in DISCRETE if k in by) + ("rew", "commands", "actions"), what)


def is_go2(env):
    from legged_gym_custom_amd import _abi
    return env.TASK_KIND == _abi.TASK_GO2


# ------------------------------------------------------------------ 1. latency is a shifted row
def latency_shift(task, n, device, steps, tmp_path=None, envs_per_wave=None):
    """envs_per_wave: lgx_set_envs_per_wave for both envs (2 on a trimesh reaches the paired terrain
    instance, which no task takes by default)."""
    base = {"noise.add_noise": False, "env.episode_length_s": short_episode}
    X = make_env(task, n, device, tmp_path, **base, **{"domain_rand.max_obs_delay_s": capacity()})
    Y = make_env(task, n, device, tmp_path, **base)
    if envs_per_wave is not None:
        X._native.set_envs_per_wave(envs_per_wave)
        Y._native.set_envs_per_wave(envs_per_wave)
    H, Pp = dims(X)
    assert X.sensor_history.shape == (n, K, Pp) and X.sensor_count.dtype == torch.int32
    assert Y.sensor_history is None and Y.obs_delay_steps is None and Y.sensor_count is None
    d = (torch.arange(n) % (K + 1))
    X.set_obs_delay(d.double().to(device) * X.dt)
    assert torch.equal(X.obs_delay_steps.cpu().long(), d)
    sens = sensor_mask(X)
    assert 0 < int(sens.sum()) < Pp
    co = float(X.cfg.normalization.clip_observations)
    X.reset()
    Y.reset()
    stagger(X, Y)
    # reset() ends with a step of its own: the first row of every env's episode
    assert torch.equal(X.sensor_count.cpu(), torch.ones(n, dtype=torch.int32))
    rows = [cur_row(Y).cpu().clone()]
    count = torch.ones(n, dtype=torch.long)
    ever_reset = torch.zeros(n, dtype=torch.bool)
    gen = torch.Generator().manual_seed(31)
    e = torch.arange(n)
    wrong_differs = 0
    for t in range(1, steps + 1):
        a = (0.3 * torch.randn(n, X.num_actions, generator=gen)).to(device)
        X.step(a.clone())
        Y.step(a.clone())
        same_physics(X, Y, f"{task} n={n} step {t}")
        rows.append(cur_row(Y).cpu().clone())
        assert float(rows[-1].abs().max()) < co  # the clip is the identity here: obs rows are the raw rows
        reset = Y.reset_buf.cpu().bool()
        ever_reset |= reset
        used = torch.where(reset, torch.zeros_like(count), count)  # rows of this episode before the step
        deff = torch.minimum(d, used)
        hist = torch.stack(rows)  # [t + 1, n, P]

        def ref(shift):
            idx = (t - deff - shift).clamp(0, t)
            back = hist[idx, e]
            return torch.where(sens.view(1, Pp), back, rows[-1])

        got = cur_row(X).cpu()
        assert torch.equal(got, ref(0)), (task, t, float((got - ref(0)).abs().max()))
        delayed = deff > 0
        if bool(delayed.any()):  # a read one step too late or too early is another row
            early, late, can = ref(-1), ref(1), delayed & (t - deff - 1 >= 0)  # (a row before the run's first: no such read)
            assert not torch.equal(got[delayed], early[delayed])
            assert not bool(can.any()) or not torch.equal(got[can], late[can])
            wrong_differs += 1
        count = used + 1
        assert torch.equal(X.sensor_count.cpu().long(), count), (task, t)
        ring = X.sensor_history.cpu()
        for j in range(K):  # the ring holds the raw rows of this episode, newest at (count - 1) % K
            have = count > j
            slot = (count - 1 - j) % K
            assert torch.equal(ring[e, slot][have], hist[t - j][have]), (task, t, j)
        # the history carries the modelled row, not the raw one
        newest = X.obs_history_buf[:, H - 1].cpu().clamp(-co, co)
        assert torch.equal(newest[~reset], got[~reset])
        if is_go2(X):
            assert torch.equal(cur_row(X, X.critic_obs_buf).cpu(), got)
    assert bool(ever_reset.any()) and not bool(ever_reset.all()), (int(ever_reset.sum()), n)
    assert wrong_differs >= steps - 1
    assert int(count.max()) > K  # the ring wrapped


# ------------------------------------------------------------------ 2. bias is an added constant
def bias_added(task, n, device, steps, tmp_path=None):
    base = {"noise.add_noise": True, "env.episode_length_s": short_episode}
    X, Y = make_env(task, n, device, tmp_path, **base), make_env(task, n, device, tmp_path, **base)
    H, Pp = dims(X)
    gen = torch.Generator().manual_seed(32)
    b = (torch.rand(n, Pp, generator=gen) - 0.5).to(device)  # on every channel: the step adds where the caller put it
    b[:, ::7] = 0.0
    assert X.obs_biases is None
    X.set_obs_bias(b)
    assert torch.equal(X.obs_biases, b) and Y.obs_biases is None and X.sensor_history is None
    co = float(X.cfg.normalization.clip_observations)
    X.reset()
    Y.reset()
    stagger(X, Y)
    ever_reset = torch.zeros(n, dtype=torch.bool)
    for t in range(steps):
        a = (0.3 * torch.randn(n, X.num_actions, generator=gen)).to(device)
        X.step(a.clone())
        Y.step(a.clone())
        same_physics(X, Y, f"{task} n={n} step {t}")
        ever_reset |= Y.reset_buf.cpu().bool()
        want = cur_row(Y) + b  # fp32 torch
        assert float(want.abs().max()) < co and float(cur_row(Y).abs().max()) < co
        assert torch.equal(cur_row(X), want), (task, t, float((cur_row(X) - want).abs().max()))
        assert torch.equal(X.obs_history_buf[:, H - 1], Y.obs_history_buf[:, H - 1] + b)
        if is_go2(X):
            assert torch.equal(cur_row(X, X.critic_obs_buf), cur_row(Y, Y.critic_obs_buf) + b)
        for name in ("priv", "est", "scan"):
            if name in bound(Y):
                assert torch.equal(bound(X)[name], bound(Y)[name]), name
    assert bool(ever_reset.any()) and not bool(ever_reset.all())


# ------------------------------------------------------------------ 3. noise scale
def noise_scale(task, n, device, steps, tmp_path=None):
    ep = {"env.episode_length_s": short_episode}
    X = make_env(task, n, device, tmp_path, **ep)
    Y = make_env(task, n, device, tmp_path, **ep)
    Z = make_env(task, n, device, tmp_path, **ep, **{"noise.add_noise": False})
    assert X.cfg.noise.add_noise and not Z.cfg.noise.add_noise
    levels = torch.tensor([0.0, 0.5, 1.0, 2.0, 4.0])
    s = levels[torch.arange(n) % 5]
    X.set_obs_noise_scale(s.to(device))
    assert Y.obs_noise_scales is None and Z.obs_noise_scales is None
    for env in (X, Y, Z):
        env.reset()
    stagger(X, Y, Z)
    gen = torch.Generator().manual_seed(33)
    worst, plain, ever_reset = 0.0, 0.0, torch.zeros(n, dtype=torch.bool)
    for t in range(steps):
        a = (0.3 * torch.randn(n, X.num_actions, generator=gen)).to(device)
        for env in (X, Y, Z):
            env.step(a.clone())
        same_physics(X, Y, f"{task} step {t} (Y)")
        same_physics(X, Z, f"{task} step {t} (Z)")
        ever_reset |= Y.reset_buf.cpu().bool()
        x, y, z = (cur_row(env).cpu() for env in (X, Y, Z))
        assert torch.equal(x[s == 1.0], y[s == 1.0]), (task, t, "scale 1 is the unbound step")
        assert torch.equal(x[s == 0.0], z[s == 0.0]), (task, t, "scale 0 is add_noise = 0")
        assert not torch.equal(y, z)
        xd, yd, zd, sd = x.double(), y.double(), z.double(), s.double().view(n, 1)
        lim = (1.0 + sd) * 2.0 ** -23 * torch.maximum(torch.maximum(xd.abs(), yd.abs()), zd.abs())
        err = (xd - (zd + sd * (yd - zd))).abs()
        assert bool((err <= lim).all()), (task, t, float((err / lim.clamp_min(1e-300)).max()))
        worst = max(worst, float((err / lim.clamp_min(1e-300)).max()))
        other = (s != 1.0)
        plain = max(plain, float(((xd - yd).abs()[other] / lim[other].clamp_min(1e-300)).max()))
    print(f"sensor noise scale {task} {device}: worst |X - (Z + s (Y - Z))| / bound {worst:.3f}; "
          f"the unscaled reference: {plain:.0f} x the bound")
    assert plain >= 100.0, plain
    assert bool(ever_reset.any()) and not bool(ever_reset.all())


# ------------------------------------------------------------------ 4. identity
def identity(task, n, device, tmp_path=None):
    ep = {"env.episode_length_s": short_episode}
    X = make_env(task, n, device, tmp_path, **ep, **{"domain_rand.sensor_model": True,
                                                     "domain_rand.max_obs_delay_s": capacity()})
    Y = make_env(task, n, device, tmp_path, **ep)
    _, Pp = dims(X)
    assert X.obs_noise_scales.shape == (n,) and X.obs_biases.shape == (n, Pp) and X.sensor_history.shape == (n, K, Pp)
    assert float(X.obs_noise_scales.min()) == 1.0 == float(X.obs_noise_scales.max())
    assert float(X.obs_biases.abs().sum()) == 0.0 and int(X.obs_delay_steps.abs().sum()) == 0
    for name in ("obs_noise_scale", "obs_bias", "obs_delay", "sensor_history", "sensor_count"):
        assert name in bound(X) and name not in bound(Y), name
    X.reset()
    Y.reset()
    stagger(X, Y)
    gen = torch.Generator().manual_seed(34)
    ever_reset = torch.zeros(n, dtype=torch.bool)
    for t in range(8):
        a = (0.5 * torch.randn(n, X.num_actions, generator=gen)).to(device)
        X.step(a.clone())
        Y.step(a.clone())
        ever_reset |= Y.reset_buf.cpu().bool()
        bx, by = bound(X), bound(Y)
        assert_equal(bx, by, [k for k in by if k in bx], f"{task} step {t}")
    assert bool(ever_reset.any()) and not bool(ever_reset.all())


def curriculum_rewrite(n, device):
    """lgx_command_curriculum on a step where the range moves (the setup of
    command_case.curriculum_redraw): neutral buffers change nothing; a bias on the command channels
    is added to the rewritten obs, critic and history command slots."""
    over = {"commands.curriculum": True, "commands.max_forward_vel": 2.0}
    on = {"domain_rand.sensor_model": True, "domain_rand.max_obs_delay_s": capacity()}
    X, Xb, Y = make_env("go2", n, device, **over, **on), make_env("go2", n, device, **over, **on), \
        make_env("go2", n, device, **over)
    assert Y.cfg.noise.add_noise  # the noise term of the rewritten slots goes through the shared helper
    H, Pp = dims(X)
    cmd = X.obs_channel_groups()["command"]
    assert (cmd.start, cmd.stop) == (5, 8)
    gen = torch.Generator().manual_seed(35)
    b = torch.zeros(n, Pp)
    b[:, cmd] = torch.rand(n, 3, generator=gen) - 0.5
    b = b.to(device)
    Xb.set_obs_bias(b)
    Xb.set_obs_noise_scale(1.0)
    reset = (torch.arange(n) % 3 != 0).to(device)
    for env in (X, Xb, Y):
        env.reset()
        env.step(torch.zeros(n, env.num_actions, device=device))
        env.reset_buf.copy_(reset)
        env._curriculum_vals.fill_(1e6)  # far past the threshold
    before = {k: t.clone() for k, t in bound(Y).items()}
    for env in (X, Xb, Y):
        env._native.command_curriculum(env.seed, int(env.max_episode_length), None, env._stream())
    bx, bb, by = bound(X), bound(Xb), bound(Y)
    assert not torch.equal(by["command_ranges"], before["command_ranges"]), "the range did not change"
    assert int((by["commands"][reset] != before["commands"][reset]).any(1).sum()) > 0  # a redraw did happen
    assert_equal(bx, by, [k for k in by if k in bx], "neutral sensor buffers through the curriculum")
    assert torch.equal(bb["commands"], by["commands"])
    r = reset
    sl = slice(H * Pp + cmd.start, H * Pp + cmd.stop)
    add = b[:, cmd]
    assert torch.equal(Xb.obs_buf[r][:, sl], Y.obs_buf[r][:, sl] + add[r])
    assert torch.equal(Xb.critic_obs_buf[r][:, sl], Y.critic_obs_buf[r][:, sl] + add[r])
    hx, hy = Xb.obs_history_buf[r][:, :, cmd], Y.obs_history_buf[r][:, :, cmd]
    assert torch.equal(hx, hy + add[r].view(-1, 1, 3))
    assert not torch.equal(Y.obs_buf[r][:, sl], before["obs"][r][:, sl])  # the slots were rewritten


# ------------------------------------------------------------------ 5. the device's backend against the host backend
def backend_vs_host(n, device):
    over = {"domain_rand.sensor_model": True, "domain_rand.max_obs_delay_s": capacity(),
            "env.episode_length_s": short_episode}
    X, Yh = make_env("go2", n, device, **over), make_env("go2", n, "cpu", **over)
    _, Pp = dims(X)
    gen = torch.Generator().manual_seed(36)
    d = torch.arange(n) * 5 % (K + 1)
    s = torch.tensor([0.0, 0.5, 1.0, 2.0, 4.0])[torch.arange(n) % 5]
    b = (torch.rand(n, Pp, generator=gen) - 0.5) * X.sensor_amplitudes.cpu() * 4.0
    for env in (X, Yh):
        env.set_obs_delay(d.double().to(env.device) * env.dt)
        env.set_obs_noise_scale(s.to(env.device))
        env.set_obs_bias(b.to(env.device))
        env.reset()
    stagger(X, Yh)
    cont = PHYSICS + ("obs", "critic", "obs_history", "sensor_history", "rew", "last_dof_vel", "last_torques", "commands")
    worst, ever_reset = {}, torch.zeros(n, dtype=torch.bool)
    for t in range(16):
        a = 0.3 * torch.randn(n, X.num_actions, generator=gen)
        copy_state(X, Yh)
        Yh.common_step_counter = X.common_step_counter
        X.step(a.to(device))
        Yh.step(a.clone())
        bx, by = bound(X), bound(Yh)
        assert_equal(bx, by, [k for k in DISCRETE if k in bx] + ["sensor_count", "obs_delay", "obs_noise_scale", "obs_bias",
                                                                 "last_actions", "actions"], f"step {t}")
        ever_reset |= X.reset_buf.cpu().bool()
        r = worst_ratio(bx, by, cont, worst)
        assert r <= 1.0, (t, r, worst)
    print(f"sensor go2 n={n} {device} vs host, all three on:", {k: f"{v:.1e}" for k, v in worst.items() if v > 0})
    assert bool(ever_reset.any()) and not bool(ever_reset.all())
    assert int(X.sensor_count.max()) > K and int(X.sensor_count.min()) >= 1
    ids = torch.arange(0, n, 3, device=X.device)
    X.reset_idx(ids)  # lgx_reset_envs empties the ring of the envs it resets
    assert int(X.sensor_count[ids].abs().sum()) == 0 and int(X.sensor_count[1::3].min()) >= 1


# ------------------------------------------------------------------ 6. setup draws
def setup_draws(device, monkeypatch):
    n = 64
    base = {"domain_rand.randomize_kp_kd": True, "domain_rand.randomize_base_mass": True,
            "domain_rand.randomize_action_delay": True, "domain_rand.action_delay_range_s": [0.0, 0.03],
            "domain_rand.randomize_motor_strength": True}
    on = dict(base, **{"domain_rand.randomize_obs_noise_scale": True, "domain_rand.obs_noise_scale_range": [0.5, 2.0],
                       "domain_rand.randomize_obs_bias": True, "domain_rand.obs_bias_level_range": [0.0, 2.0],
                       "domain_rand.randomize_obs_delay": True, "domain_rand.obs_delay_range_s": [0.0, 0.04]})
    X, Y = make_env("go2", n, device, **on), make_env("go2", n, device, **base)
    for name in ("friction", "mass_params", "kp_kd", "action_delay", "motor_strength"):  # existing draws keep their values
        assert torch.equal(bound(X)[name], bound(Y)[name]), name
    assert Y.obs_noise_scales is None and Y.obs_biases is None and Y.obs_delay_steps is None and Y.sensor_count is None
    sc, bs, dl = X.obs_noise_scales, X.obs_biases, X.obs_delay_steps
    _, Pp = dims(X)
    assert sc.shape == (n,) and float(sc.min()) >= 0.5 and float(sc.max()) <= 2.0 and len(sc.unique()) > n // 2
    assert dl.dtype == torch.int32 and int(dl.min()) >= 0 and int(dl.max()) <= 2 and len(dl.unique()) == 3
    assert X.sensor_history.shape == (n, 2, Pp)  # round(0.04 / 0.02)
    amp, sens = X.sensor_amplitudes, sensor_mask(X).to(device)
    assert bs.shape == (n, Pp) and float(bs[:, ~sens].abs().sum()) == 0.0 and bool((bs.abs() <= 2.0 * amp).all())
    assert int((bs[:, sens] != 0).sum()) > n * int(sens.sum()) // 2
    import torch.distributed as dist
    for rank in (0, 1):  # two ranks of 32 envs draw rows [0, 32) and [32, 64) of the single-process draw
        monkeypatch.setattr(dist, "is_initialized", lambda: True)
        monkeypatch.setattr(dist, "get_rank", lambda group=None, rank=rank: rank)
        monkeypatch.setattr(dist, "get_world_size", lambda group=None: 2)
        S = make_env("go2", n // 2, device, **on)
        monkeypatch.undo()
        sl = slice(rank * n // 2, (rank + 1) * n // 2)
        assert S.env_id_offset == rank * n // 2 and S.num_envs_total == n
        assert torch.equal(S.obs_noise_scales, sc[sl]) and torch.equal(S.obs_biases, bs[sl])
        assert torch.equal(S.obs_delay_steps, dl[sl]) and torch.equal(S.motor_strengths, X.motor_strengths[sl])


def layouts_and_amplitudes():
    """The layout functions, obs_channel_groups, sensor_amplitudes and obs_bias_from_physical."""
    import numpy as np
    import pytest
    from legged_gym_custom_amd import params as prm
    from legged_gym_custom_amd.envs import task_registry_configs
    env = make_env("go2", 8, "cpu")
    g = env.obs_channel_groups()
    assert {k: (v.start, v.stop) for k, v in g.items()} == {
        "ang_vel": (0, 3), "roll_pitch": (3, 5), "command": (5, 8), "dof_pos": (8, 20), "dof_vel": (20, 32),
        "actions": (32, 44), "phase": (44, 52)}
    cfg = env.cfg
    ns, sc, lvl = cfg.noise.noise_scales, cfg.normalization.obs_scales, cfg.noise.noise_level
    amp = prm.sensor_amplitudes(cfg, True)
    want = np.zeros(52, dtype=np.float32)
    want[0:3] = ns.ang_vel * lvl * sc.ang_vel
    want[3:5] = ns.imu * lvl
    want[8:20] = ns.dof_pos * lvl * sc.dof_pos
    want[20:32] = ns.dof_vel * lvl * sc.dof_vel
    assert np.array_equal(amp, want) and np.array_equal(env.sensor_amplitudes.numpy(), want)
    assert not np.array_equal(amp, prm.noise_vector(cfg, True))  # the Go2 noise slots are shifted by one
    b = env.obs_bias_from_physical(ang_vel=0.1, dof_pos=torch.arange(12.0), roll_pitch=torch.ones(8, 2))
    assert b.shape == (8, 52) and torch.equal(b[:, 0:3], torch.full((8, 3), 0.1 * sc.ang_vel))
    assert torch.equal(b[:, 8:20], (torch.arange(12.0) * sc.dof_pos).expand(8, 12)) and float(b[:, 3:5].min()) == 1.0
    assert float(b[:, 5:8].abs().sum() + b[:, 20:].abs().sum()) == 0.0
    for bad in ({"lin_vel": 0.1}, {"gravity": 0.1}, {"heights": 0.1}, {"command": 0.1}, {"nonsense": 1.0},
                {"ang_vel": torch.ones(4)}, {"dof_vel": float("nan")}):
        with pytest.raises(ValueError):
            env.obs_bias_from_physical(**bad)
    acfg = task_registry_configs("anymal_c_rough")[0]
    ga = prm.proprio_channel_groups(acfg, False)
    assert {k: (v.start, v.stop) for k, v in ga.items()} == {
        "lin_vel": (0, 3), "ang_vel": (3, 6), "gravity": (6, 9), "command": (9, 12), "dof_pos": (12, 24),
        "dof_vel": (24, 36), "actions": (36, 48), "heights": (48, 235)}
    assert np.array_equal(prm.sensor_amplitudes(acfg, False), prm.noise_vector(acfg, False))  # LEGGED: no shift


# ------------------------------------------------------------------ 7. refusals and clamps
def refusals(device):
    import pytest
    from legged_gym_custom_amd import _abi, _native
    with pytest.raises(ValueError, match="LGX_MAX_SENSOR_HISTORY"):
        make_env("go2", 8, device, **{"domain_rand.max_obs_delay_s": capacity(5)})
    make_env("go2", 8, device, **{"domain_rand.max_obs_delay_s": capacity(4)})  # K = 4 is allowed
    plain = make_env("go2", 8, device)
    _, Pp = dims(plain)
    P5 = _abi.TaskParams.from_buffer_copy(plain.task_params)
    P5.sensor_history_len = 5
    with pytest.raises(_native.LgxError, match="sensor_history_len outside"):
        _native.NativeEnv(plain._native.model, P5, plain.sim_device_id)
    with pytest.raises(ValueError, match="without sensing latency"):
        plain.set_obs_delay(0.02)

    def refused(match, **attrs):
        for k, v in attrs.items():
            setattr(plain, k, v)
        with pytest.raises(_native.LgxError, match=match):
            plain._bind()
        for k in attrs:
            setattr(plain, k, None)

    i32 = lambda *s: torch.zeros(*s, dtype=torch.int32, device=device)  # noqa: E731
    f32 = lambda *s: torch.zeros(*s, device=device)  # noqa: E731
    refused("obs_delay needs sensor_history", obs_delay_steps=i32(8))
    refused("obs_delay needs sensor_history", obs_delay_steps=i32(8), sensor_history=f32(8, 1, Pp), sensor_count=i32(8))  # K = 0
    refused("sensor_history needs sensor_count", sensor_history=f32(8, 1, Pp))
    refused("sensor_count needs sensor_history", sensor_count=i32(8))
    refused("sensor_history with params.sensor_history_len = 0", sensor_history=f32(8, 1, Pp), sensor_count=i32(8))
    plain._bind()
    env = make_env("go2", 8, device, **{"domain_rand.max_obs_delay_s": capacity(2)})
    env.set_obs_delay(0.04)  # 2 control steps: the capacity
    assert int(env.obs_delay_steps.min()) == 2
    for bad in (0.06, -0.02, float("nan"), torch.zeros(7)):
        with pytest.raises(ValueError):
            env.set_obs_delay(bad)
    assert int(env.obs_delay_steps.min()) == 2 == int(env.obs_delay_steps.max())  # a refused value writes nothing
    env.set_obs_noise_scale(2.0)
    for bad in (-0.1, float("inf"), float("nan"), torch.ones(7), torch.ones(8, 2)):
        with pytest.raises(ValueError):
            env.set_obs_noise_scale(bad)
    assert float(env.obs_noise_scales.min()) == 2.0 == float(env.obs_noise_scales.max())
    env.set_obs_bias(torch.full((Pp,), 0.25))
    for bad in (torch.ones(Pp + 1), torch.ones(7, Pp), torch.full((8, Pp), float("inf")), 0.5):
        with pytest.raises(ValueError):
            env.set_obs_bias(bad)
    assert float(env.obs_biases.min()) == 0.25 == float(env.obs_biases.max())
    # the step clamps what the Python layer would refuse: a raw out-of-range tensor behaves as its clamp
    over = {"domain_rand.max_obs_delay_s": capacity(2), "noise.add_noise": False}
    raw, ref = make_env("go2", 8, device, **over), make_env("go2", 8, device, **over)
    ref.set_obs_delay(0.04)
    raw.obs_delay_steps.fill_(1 << 30)
    raw.obs_delay_steps[::2] = -5
    ref.obs_delay_steps[::2] = 0
    gen = torch.Generator().manual_seed(37)
    for e in (raw, ref):
        e.reset()
    for _ in range(5):
        a = torch.randn(8, raw.num_actions, generator=gen).to(device)
        raw.step(a.clone())
        ref.step(a.clone())
        assert_equal(bound(raw), bound(ref), PHYSICS + ("obs", "obs_history", "sensor_history", "sensor_count"), "clamped delay")
    assert not torch.equal(cur_row(raw)[1::2], cur_row(raw)[::2])


def captured_refusal(device):
    """The allocating first call of a setter is refused once a step of the env has been captured."""
    import pytest
    env = make_env("go2", 8, device)
    env.reset()
    a = torch.zeros(8, env.num_actions, device=device)
    env.step(a)
    if device == "cpu":
        env._captured = True  # (the host backend captures nothing: the flag a capture sets)
    else:
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        csc = env.common_step_counter
        with torch.no_grad(), torch.cuda.graph(g):
            env.step(a)
        env.common_step_counter = csc
        assert env._captured
    _, Pp = dims(env)
    with pytest.raises(RuntimeError, match="captured"):
        env.set_obs_noise_scale(2.0)
    with pytest.raises(RuntimeError, match="captured"):
        env.set_obs_bias(torch.zeros(Pp))
    assert env.obs_noise_scales is None and env.obs_biases is None


# ------------------------------------------------------------------ 8. evaluator
def evaluator(device):
    """tests/test_gpu_eval.py's setup (66 envs, a 10-step episode) with the sensor test."""
    import pytest
    import eval_case as E
    from legged_gym_custom_amd.utils.evaluator import REPORT_KEYS, PolicyEvaluator

    def make(**over):
        env, tcfg, args = E.make_env("go2", 66, device, **{"env.episode_length_s": 0.19, **over})
        return PolicyEvaluator(env, E.make_runner(env, tcfg, args))

    on = {"domain_rand.sensor_model": True, "domain_rand.max_obs_delay_s": 0.04}
    a, b, plain = make(**on), make(**on), make()
    env = a.env
    own_s = (0.5 + torch.arange(66) % 3).to(device)
    own_d = (torch.arange(66) % 3).to(torch.int32).to(device)
    own_b = (torch.arange(66 * 52).view(66, 52) % 5).float().to(device) * 1e-3
    env.set_obs_noise_scale(own_s)
    env.set_obs_bias(own_b)
    env.obs_delay_steps.copy_(own_d)
    # one bin of neutral values: the per-env records of a plain run()
    plain.run()
    one = a.run_sensor_test()
    assert one["delay_steps"] == [0] and one["noise"] == [1.0] and one["bias"] == [0.0]
    assert torch.equal(env.sensor_eval_acc, plain.env.eval_acc) and torch.equal(env.sensor_eval_status, plain.env.eval_status)
    assert set(REPORT_KEYS) == set(one["total"]) == set(one["bins"][0][0][0])
    for k in REPORT_KEYS:
        assert one["total"][k] == plain.report(plain.last_cells)["total"][k], k
    # the env's own values are back
    assert torch.equal(env.obs_noise_scales, own_s) and torch.equal(env.obs_biases, own_b)
    assert torch.equal(env.obs_delay_steps, own_d)
    grid = dict(noise=(0.0, 2.0), bias=(0.0, 3.0), delay_s=(0.0, 0.04))
    ra = a.run_sensor_test(**grid)
    assert ra["graph"] is (device != "cpu") and ra["delay_steps"] == [0, 2] and ra["total"]["running"] == 0
    assert len(ra["bins"]) == 2 and all(len(p) == 2 and all(len(r) == 2 for r in p) for p in ra["bins"])
    sizes = [c["episodes"] + c["running"] for p in ra["bins"] for r in p for c in r]
    assert sum(sizes) == 66 and max(sizes) - min(sizes) <= 1
    assert ra["total"]["episodes"] == 66
    cells = a.last_cells.clone()
    assert cells.shape == (2, 4, 12)
    rb = b.run_sensor_test(graph=False, **grid)
    assert rb["graph"] is False and torch.equal(cells, b.last_cells)  # graph replay == the eager loop
    assert torch.equal(env.obs_noise_scales, own_s) and torch.equal(env.obs_biases, own_b)
    assert torch.equal(env.obs_delay_steps, own_d)
    assert float(b.env.obs_noise_scales.min()) == 1.0 and float(b.env.obs_biases.abs().sum()) == 0.0
    graph = a._sensor_graph
    a.run_sensor_test(noise=(1.0, 4.0), bias=(1.0, 2.0), delay_s=(0.02, 0.04))  # other levels, the same shape
    assert a._sensor_graph is graph
    if device != "cpu":
        assert graph is not None
        a.run_sensor_test(noise=(1.0,), bias=(1.0, 2.0), delay_s=(0.02, 0.04))
        assert a._sensor_graph is not graph  # another shape: its own capture
        with pytest.raises(RuntimeError, match="captured"):
            plain.run_sensor_test(noise=(1.0, 2.0))  # allocating now would re-bind under plain's captured loop
    rg = a.run_sensor_test(gait=True, **grid)
    assert rg["bins"][1][1][1]["gait"]["envs"] == rg["bins"][1][1][1]["episodes"] and "gait" in rg["total"]
    for bad in (dict(noise=()), dict(bias=[]), dict(delay_s=()), dict(noise=(-1.0,)), dict(bias=(float("nan"),)),
                dict(delay_s=(float("inf"),)), dict(delay_s=(0.06,))):
        with pytest.raises(ValueError):
            a.run_sensor_test(**bad)
    with pytest.raises(ValueError):
        plain.run_sensor_test(delay_s=(0.02,))  # no capacity
    quiet = make(**on, **{"noise.add_noise": False})
    with pytest.raises(ValueError, match="add_noise"):
        quiet.run_sensor_test(noise=(0.0, 1.0))
    assert torch.equal(env.obs_noise_scales, own_s) and torch.equal(env.obs_delay_steps, own_d)


def evaluate_cli_document(device, tmp_path):
    """legged_gym/scripts/evaluate.py (a child process: it edits the registry's configs) on a checkpoint of
    randomly initialised networks: the sensor test's document."""
    import json
    import os
    import subprocess
    import sys
    import eval_case as E
    from legged_gym_custom_amd.envs import task_registry
    repo = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env, tcfg, args = E.make_env("go2", 8, "cpu")
    runner, tcfg = task_registry.make_alg_runner(env, name="go2", args=args, train_cfg=tcfg,
                                                 log_root=os.path.join(str(tmp_path), tcfg.runner.experiment_name))
    os.makedirs(runner.log_dir, exist_ok=True)
    runner.save(os.path.join(runner.log_dir, "model_0.pt"))
    penv = dict(os.environ, PYTHONPATH=repo, PYTHONDONTWRITEBYTECODE="1", LGX_LOG_ROOT=str(tmp_path), OMP_NUM_THREADS="4")
    r = subprocess.run([sys.executable, os.path.join(repo, "legged_gym", "scripts", "evaluate.py"), "--eval_steps=3",
                        "--obs_noise", "0,2", "--obs_delay_ms", "0,20", "--task=go2", f"--sim_device={device}",
                        f"--rl_device={device}", "--num_envs=8", "--headless"],
                       cwd=str(tmp_path), env=penv, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    doc = json.loads(r.stdout.strip().splitlines()[-1])
    assert doc["task"] == "go2" and doc["policy"] == "student" and doc["num_steps"] == 3
    assert doc["noise"] == [0.0, 2.0] and doc["bias"] == [0.0] and doc["delay_s"] == [0.0, 0.02]
    assert doc["delay_steps"] == [0, 1]
    assert len(doc["bins"]) == 2 and all(len(p) == 1 and len(p[0]) == 2 for p in doc["bins"])
    out = os.path.join(os.path.dirname(doc["checkpoint"]), "eval_student_sensors.json")
    assert os.path.dirname(doc["checkpoint"]).startswith(str(tmp_path))
    with open(out) as f:
        assert json.load(f) == doc


# ------------------------------------------------------------------ 10. training smoke
def training_smoke(device, num_steps_per_env=None):
    import eval_case as E
    over = {"domain_rand.randomize_obs_noise_scale": True, "domain_rand.obs_noise_scale_range": [0.5, 2.0],
            "domain_rand.randomize_obs_bias": True, "domain_rand.obs_bias_level_range": [0.0, 2.0],
            "domain_rand.randomize_obs_delay": True, "domain_rand.obs_delay_range_s": [0.0, 0.04]}
    env, tcfg, args = E.make_env("go2", 64, device, **over)
    assert int(env.obs_delay_steps.max()) > 0 and float(env.obs_biases.abs().sum()) > 0
    if num_steps_per_env:
        tcfg.runner.num_steps_per_env = num_steps_per_env
    runner = E.make_runner(env, tcfg, args)
    runner.learn(num_learning_iterations=2, init_at_random_ep_len=True)
    if device != "cpu":
        assert env.graph_capturable and len(runner._graphs) > 0  # the rollout was captured and replayed
    assert torch.isfinite(env.obs_buf).all() and torch.isfinite(env.root_states).all()
    assert torch.isfinite(env.sensor_history).all()
    assert all(torch.isfinite(p).all() for p in runner.alg.actor_critic.parameters())
    ran = 2 * int(tcfg.runner.num_steps_per_env) + 1  # (+ the step reset() ends with)
    assert int(env.sensor_count.min()) >= 1 and int(env.sensor_count.max()) <= ran
    assert math.isfinite(float(env.sensor_history.abs().sum())) and float(env.sensor_history.abs().sum()) > 0
