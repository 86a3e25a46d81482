"""Shared by tests/test_gpu_scan.py (device "cuda:0") and tests/test_scan_host.py (the same bodies
on the host backend): the per-env height-scan model (include/lgx.h, ABI 17): noise, dropout, map
offset and latency on the Go2 task kind's scan.

The feature has no oracle. As tests/sensor_case.py does, every test reduces feature-on behaviour to
feature-off behaviour, which the oracle and the golden fixtures pin. Env X (feature) and env Y
(plain) are built with the same seed and fed the same scripted actions; the model touches `scan`
only, so every other bound buffer of X equals Y's bit for bit at every step (asserted), and
  * a latency of d control steps is Y's scan row of d steps ago (never across a reset): bit-exact;
  * noise is clip(Y + (2u - 1) amp) in np.float32 with u recomputed from oracle/philox.py's
    philox4x32_10 on stream 3: within 2^-23 absolute (one fp32 ulp at the clip limit 1, which
    covers one fused rounding of product and sum); both backends build without contraction, so
    bit equality is asserted as well and which of the two held is printed;
  * the lost points are exactly {i : u' < p} and hold the fill value bit for bit;
  * an xy offset is the scan of a plain env whose height_points hold the fp32 sums: bit-exact;
  * dz is clip(np.float32(Y + dz)): bit-exact.
Resets happen inside every run: the episode is 20 steps long and the episode lengths are staggered
in place in both envs, so a third of the envs time out within the first steps."""
import numpy as np
import torch

from actuator_case import assert_equal, bound, copy_state, make_env
from sensor_case import short_episode, stagger

K = 3  # control steps of scan history in the latency tests
CASES = [("go2", 64, None, 10), ("go2", 63, None, 10), ("go2_parkour", 64, None, 8), ("go2_parkour", 64, 2, 8)]
IDS = [f"{t}-{n}" + (f"-epw{w}" if w else "") for t, n, w, _ in CASES]
SCAN_BUFFERS = ("scan_noise", "scan_dropout", "scan_offset", "scan_delay", "scan_history")
STREAM = 3  # LGX_SCAN_STREAM
EP = {"env.episode_length_s": short_episode}


def capacity(k=K):
    """domain_rand.max_scan_delay_s for k control steps of scan history."""
    return lambda cfg: k * cfg.control.decimation * cfg.sim.dt


ON = {"domain_rand.scan_model": True, "domain_rand.max_scan_delay_s": capacity()}


def pair(task, n, device, epw, x_over, y_over=None):
    X = make_env(task, n, device, **EP, **x_over)
    Y = make_env(task, n, device, **EP, **(y_over or {}))
    if epw is not None:
        X._native.set_envs_per_wave(epw)
        Y._native.set_envs_per_wave(epw)
    return X, Y


def start(*envs):
    """reset(), the staggered episode lengths and, on a terrain, every robot moved 2 to 3 m forward
    in place: the spawn platform is flat as far as the scan reaches, out there the scan has relief
    (asserted in offset_xy). An env that resets inside the run returns to its platform."""
    for env in envs:
        env.reset()
    stagger(*envs)
    if envs[0].cfg.terrain.mesh_type != "plane":
        for env in envs:
            env.root_states[:, 0] += (2.0 + 0.25 * (torch.arange(env.num_envs) % 5)).to(env.device)


def actions(gen, env):
    return (0.3 * torch.randn(env.num_envs, env.num_actions, generator=gen)).to(env.device)


def others_equal(X, Y, what):
    """Every buffer both envs have bound, except scan: bit for bit (obs, the critic with its scan
    slots, priv, est, measured_heights, rew and the physics state among them)."""
    bx, by = bound(X), bound(Y)
    names = [k for k in by if k in bx and k != "scan" and k != "sensor_history" and k != "sensor_count"]
    for must in ("obs", "critic", "priv", "est", "rew", "root_states", "dof_state", "measured_heights"):
        assert must in names, must
    assert_equal(bx, by, names, what)


def scan_uniforms(env, step, first_slot, count):
    """[n, count] float32: slots first_slot .. first_slot + count of the scan model's Philox stream
    for the step number `step`, from oracle/philox.py (block = slot >> 2, word = slot & 3)."""
    from oracle import philox
    ids = np.arange(env.num_envs, dtype=np.uint32) + np.uint32(env.env_id_offset)
    k0, k1 = env.seed & 0xFFFFFFFF, (env.seed >> 32) & 0xFFFFFFFF
    out = np.empty((env.num_envs, count), dtype=np.float32)
    b0, b1 = first_slot >> 2, (first_slot + count - 1) >> 2
    for b in range(b0, b1 + 1):
        words = philox.philox4x32_10(ids, np.uint32(step & 0xFFFFFFFF), np.uint32(b | (STREAM << 16)),
                                     np.uint32((step >> 32) & 0xFFFFFFFF), k0, k1)
        for w in range(4):
            s = 4 * b + w - first_slot
            if 0 <= s < count:
                out[:, s] = philox.to_uniform(words[w])
    return out


def critic_scan(env):
    S = env.num_scan_obs
    return env.critic_obs_buf[:, -S:]


# ------------------------------------------------------------------ 1. identity
def identity(task, n, device, epw, steps):
    X, Y = pair(task, n, device, epw, ON)
    S = X.num_scan_obs
    assert X.scan_noise_amps.shape == (n,) and X.scan_dropouts.shape == (n, 2) and X.scan_offsets.shape == (n, 3)
    assert X.scan_delay_steps.dtype == torch.int32 and X.scan_history.shape == (n, K, S)
    assert float(X.scan_noise_amps.abs().sum()) == 0.0 and float(X.scan_dropouts[:, 0].abs().sum()) == 0.0
    assert float(X.scan_offsets.abs().sum()) == 0.0 and int(X.scan_delay_steps.abs().sum()) == 0
    for name in SCAN_BUFFERS:
        assert name in bound(X) and name not in bound(Y), name
    assert Y.scan_history is None and Y.scan_noise_amps is None and "sensor_count" not in bound(Y)
    start(X, Y)
    gen = torch.Generator().manual_seed(41)
    ever_reset = torch.zeros(n, dtype=torch.bool)
    for t in range(steps):
        a = actions(gen, X)
        X.step(a.clone())
        Y.step(a.clone())
        ever_reset |= Y.reset_buf.cpu().bool()
        bx, by = bound(X), bound(Y)
        assert "scan" in by
        assert_equal(bx, by, [k for k in by if k in bx], f"{task} n={n} step {t}")
    assert bool(ever_reset.any()) and not bool(ever_reset.all())


# ------------------------------------------------------------------ 2. everything on: only scan moves
def all_on(env, gen=None):
    """Noise, dropout, an xy and z offset and a latency on every env, in varied amounts."""
    n, dev = env.num_envs, env.device
    e = torch.arange(n)
    env.set_scan_noise(torch.tensor([0.0, 0.02, 0.05, 0.6])[e % 4].to(dev))
    env.set_scan_dropout(torch.tensor([0.0, 0.1, 0.5])[e % 3].to(dev), torch.tensor([1.0, -0.25])[e % 2].to(dev))
    env.set_scan_offset(torch.tensor([0.0, 0.25, -0.5])[e % 3].to(dev), torch.tensor([0.0, -0.125])[e % 2].to(dev),
                        torch.tensor([0.0, 0.03125, -0.7])[(e // 2) % 3].to(dev))
    env.set_scan_delay((e * 5 % (K + 1)).double().to(dev) * env.dt)


def others_untouched(task, n, device, epw, steps):
    X, Y = pair(task, n, device, epw, ON)
    all_on(X)
    start(X, Y)
    gen = torch.Generator().manual_seed(42)
    ever_reset, differs = torch.zeros(n, dtype=torch.bool), 0
    for t in range(steps):
        a = actions(gen, X)
        X.step(a.clone())
        Y.step(a.clone())
        ever_reset |= Y.reset_buf.cpu().bool()
        others_equal(X, Y, f"{task} n={n} step {t}")
        assert torch.equal(critic_scan(X), critic_scan(Y))  # the privileged copy stays clean
        co = float(X.cfg.normalization.clip_observations)
        assert torch.equal(critic_scan(Y), Y.scan_obs_buf.clamp(-co, co))
        differs += int(not torch.equal(X.scan_obs_buf, Y.scan_obs_buf))
        assert float(X.scan_obs_buf.abs().max()) <= 1.0
    assert differs == steps
    assert bool(ever_reset.any()) and not bool(ever_reset.all())


# ------------------------------------------------------------------ 3. latency is a shifted row
def latency_shift(task, n, device, epw, steps):
    X, Y = pair(task, n, device, epw, {"domain_rand.max_scan_delay_s": capacity()})
    S = X.num_scan_obs
    assert X.scan_history.shape == (n, K, S) and X.sensor_count.dtype == torch.int32
    assert X.scan_noise_amps is None and X.scan_offsets is None  # only the latency's buffers
    d = torch.arange(n) % (K + 1)
    X.set_scan_delay(d.double().to(device) * X.dt)
    assert torch.equal(X.scan_delay_steps.cpu().long(), d) and int(d.max()) == K
    start(X, Y)
    # reset() ends with a step of its own: the first row of every env's episode
    assert torch.equal(X.sensor_count.cpu(), torch.ones(n, dtype=torch.int32))
    rows = [Y.scan_obs_buf.cpu().clone()]
    count = torch.ones(n, dtype=torch.long)
    ever_reset = torch.zeros(n, dtype=torch.bool)
    gen = torch.Generator().manual_seed(43)
    e = torch.arange(n)
    wrong_differs = 0
    for t in range(1, steps + 1):
        a = actions(gen, X)
        X.step(a.clone())
        Y.step(a.clone())
        others_equal(X, Y, f"{task} n={n} step {t}")
        rows.append(Y.scan_obs_buf.cpu().clone())
        reset = Y.reset_buf.cpu().bool()
        ever_reset |= reset
        used = torch.where(reset, torch.zeros_like(count), count)  # rows of this episode before the step
        deff = torch.minimum(d, used)
        hist = torch.stack(rows)  # [t + 1, n, S]
        got = X.scan_obs_buf.cpu()
        want = hist[(t - deff).clamp(0, t), e]
        assert torch.equal(got, want), (task, t, float((got - want).abs().max()))
        delayed = deff > 0
        if bool(delayed.any()):  # a read one step too early is another row
            early = hist[(t - deff + 1).clamp(0, t), e]
            wrong_differs += int(not torch.equal(got[delayed], early[delayed]))
        count = used + 1
        assert torch.equal(X.sensor_count.cpu().long(), count), (task, t)
        ring = X.scan_history.cpu()
        for j in range(K):  # the ring holds the raw rows of this episode, newest at (count - 1) % K
            have = count > j
            assert torch.equal(ring[e, (count - 1 - j) % K][have], hist[t - j][have]), (task, t, j)
    assert bool(ever_reset.any()) and not bool(ever_reset.all()), (int(ever_reset.sum()), n)
    assert wrong_differs >= steps - 2
    assert int(count.max()) > K  # the ring wrapped


# ------------------------------------------------------------------ 4. noise
def noise(task, n, device, epw, steps):
    X, Y = pair(task, n, device, epw, {"domain_rand.scan_model": True})
    S = X.num_scan_obs
    amp = torch.tensor([0.0, 0.02, 0.05, 0.5, 2.0])[torch.arange(n) % 5]  # (2.0: the clip acts)
    X.set_scan_noise(amp.to(device))
    start(X, Y)
    gen = torch.Generator().manual_seed(44)
    ampn = amp.numpy().astype(np.float32).reshape(n, 1)
    worst, exact, clipped, ever_reset = 0.0, True, 0, torch.zeros(n, dtype=torch.bool)
    one, two = np.float32(1.0), np.float32(2.0)
    for t in range(steps):
        a = actions(gen, X)
        step = int(X._step_dev.item())  # the number the step is about to read
        X.step(a.clone())
        Y.step(a.clone())
        others_equal(X, Y, f"{task} n={n} step {t}")
        ever_reset |= Y.reset_buf.cpu().bool()
        u = scan_uniforms(X, step, 0, S)
        clean = Y.scan_obs_buf.cpu().numpy()
        assert clean.dtype == np.float32 and u.dtype == np.float32
        want = np.clip(clean + (two * u - one) * ampn, -one, one)
        assert want.dtype == np.float32
        got = X.scan_obs_buf.cpu().numpy()
        quiet = (amp == 0.0).numpy()
        assert np.array_equal(got[quiet].view(np.uint32), clean[quiet].view(np.uint32))  # amp 0: the bits of the clean scan
        err = float(np.abs(got.astype(np.float64) - want.astype(np.float64)).max())
        worst = max(worst, err)
        exact &= bool(np.array_equal(got.view(np.uint32), want.view(np.uint32)))
        clipped += int((np.abs(want) == 1.0).sum())
        assert err <= 2.0 ** -23, (task, t, err)
        assert float(np.abs(got[~quiet] - clean[~quiet]).max()) > 1e-3  # (the noise is there)
    print(f"scan noise {task} n={n} {device}: worst |scan - ref| {worst:.3e} (bound 2^-23 = {2.0 ** -23:.3e}); "
          f"bit equality {'held' if exact else 'did NOT hold'}; {clipped} clipped values")
    assert exact, "both backends build with -ffp-contract=off: product and sum round separately"
    assert clipped > 0
    assert bool(ever_reset.any()) and not bool(ever_reset.all())


# ------------------------------------------------------------------ 5. dropout
def dropout(task, n, device, epw, steps):
    from legged_gym_custom_amd import _abi
    X, Y = pair(task, n, device, epw, {"domain_rand.scan_model": True})
    S = X.num_scan_obs
    e = torch.arange(n)
    p = torch.tensor([0.0, 0.1, 0.5, 1.0])[e % 4]
    fill = torch.tensor([1.0, -0.75, 0.3])[e % 3]
    X.set_scan_dropout(p.to(device), fill.to(device))
    start(X, Y)
    gen = torch.Generator().manual_seed(45)
    lost_total = 0
    for t in range(steps):
        a = actions(gen, X)
        step = int(X._step_dev.item())
        X.step(a.clone())
        Y.step(a.clone())
        others_equal(X, Y, f"{task} n={n} step {t}")
        ud = torch.from_numpy(scan_uniforms(X, step, _abi.MAX_HEIGHT_POINTS, S))
        lost = ud < p.view(n, 1)
        assert not bool(lost[p == 0.0].any()) and bool(lost[p == 1.0].all())
        want = torch.where(lost, fill.view(n, 1).expand(n, S), Y.scan_obs_buf.cpu())
        got = X.scan_obs_buf.cpu()
        assert torch.equal(got.view(torch.int32), want.view(torch.int32)), (task, t)
        # where the clean value is not the fill value itself (over a gap the clean scan clips to 1),
        # the lost set can be read back from the scan
        clean = Y.scan_obs_buf.cpu()
        free = clean != fill.view(n, 1)
        assert int(free.sum()) > n * S // 2
        assert torch.equal((got == fill.view(n, 1))[free], lost[free])
        lost_total += int(lost.sum())
    mid = (p == 0.5) | (p == 0.1)
    assert 0 < lost_total < steps * n * S and bool(mid.any())


# ------------------------------------------------------------------ 6. offset
def offset_xy(n, device, epw, steps, task="go2_parkour"):
    """The scan of X with (dx, dy, 0) against the scan of a plain env whose params.height_points hold
    the fp32 sums, written into the params struct before lgx_create (a fresh native env on the
    plain env's buffers)."""
    from legged_gym_custom_amd import _abi, _native
    dx, dy = 0.25, -0.375  # at least one horizontal_scale each
    X, Y = pair(task, n, device, epw, {"domain_rand.scan_model": True})
    Z = make_env(task, n, device, **EP)  # the shifted plain env
    hs = float(X.cfg.terrain.horizontal_scale)
    assert abs(dx) >= hs and abs(dy) >= hs
    P = _abi.TaskParams.from_buffer_copy(Z.task_params)
    NP = int(P.num_height_points)
    pts = np.ctypeslib.as_array(P.height_points).reshape(-1, 2)
    pts[:NP, 0] = (pts[:NP, 0].astype(np.float32) + np.float32(dx)).astype(np.float32)
    pts[:NP, 1] = (pts[:NP, 1].astype(np.float32) + np.float32(dy)).astype(np.float32)
    keep = dict(Z._native._keep)
    Z._native = _native.NativeEnv(Z._native.model, P, Z.sim_device_id)
    Z.task_params = P
    Z._bind()
    if epw is not None:
        Z._native.set_envs_per_wave(epw)
    assert set(bound(Z)) == {k for k, v in keep.items() if not k.startswith("_") and torch.is_tensor(v)}
    sel = (torch.arange(n) % 3 != 0)  # a third of the envs keep a zero offset: the staged heights
    X.set_scan_offset(torch.where(sel, dx, 0.0).to(device), torch.where(sel, dy, 0.0).to(device), 0.0)
    start(X, Y, Z)
    gen = torch.Generator().manual_seed(46)
    differs, relief, ever_reset = 0, 0, torch.zeros(n, dtype=torch.bool)
    phys = ("root_states", "dof_state", "reset", "episode_length")
    for t in range(steps):
        a = actions(gen, X)
        for env in (X, Y, Z):
            env.step(a.clone())
        others_equal(X, Y, f"{task} n={n} step {t}")
        assert_equal(bound(Z), bound(Y), phys, f"shifted plain env, step {t}")  # the same trajectory
        ever_reset |= Y.reset_buf.cpu().bool()
        x, y, z = X.scan_obs_buf.cpu(), Y.scan_obs_buf.cpu(), Z.scan_obs_buf.cpu()
        assert torch.equal(x[sel].view(torch.int32), z[sel].view(torch.int32)), (task, t, float((x[sel] - z[sel]).abs().max()))
        assert torch.equal(x[~sel].view(torch.int32), y[~sel].view(torch.int32))
        differs += int(not torch.equal(x[sel], y[sel]))
        relief += int(((y.max(1).values - y.min(1).values) > 1e-3).sum())
    assert differs >= steps // 2 and relief >= n, (differs, relief)  # the offset rows differ from the clean ones
    assert bool(ever_reset.any()) and not bool(ever_reset.all())


def offset_z(task, n, device, epw, steps):
    X, Y = pair(task, n, device, epw, {"domain_rand.scan_model": True})
    dz = torch.tensor([0.0, 0.03, -0.11, 0.9, -1.5])[torch.arange(n) % 5]
    X.set_scan_offset(0.0, 0.0, dz.to(device))
    start(X, Y)
    gen = torch.Generator().manual_seed(47)
    for t in range(steps):
        a = actions(gen, X)
        X.step(a.clone())
        Y.step(a.clone())
        others_equal(X, Y, f"{task} n={n} step {t}")
        clean = Y.scan_obs_buf.cpu().numpy()
        want = np.clip(clean + dz.numpy().astype(np.float32).reshape(n, 1), np.float32(-1.0), np.float32(1.0))
        got = X.scan_obs_buf.cpu().numpy()
        assert want.dtype == np.float32 and np.array_equal(got.view(np.uint32), want.view(np.uint32)), (task, t)
    assert not np.array_equal(got, clean) and float(np.abs(want).max()) == 1.0


# ------------------------------------------------------------------ 7. the device's backend against the host backend
def backend_vs_host(n, device, task="go2_parkour"):
    """All four effects on. The two backends' physics agree to rounding only (tests/actuator_case.py),
    and the scan inherits root_z from it, so the comparison is made on the step's post-physics half,
    which forms the scan: X runs whole steps; after each, every bound buffer of X is copied to the
    host env and both run lgx_post_physics on that state with the same step number. scan, the ring
    and the count: bit for bit."""
    X, Yh = make_env(task, n, device, **EP, **ON), make_env(task, n, "cpu", **EP, **ON)
    for env in (X, Yh):
        all_on(env)
    start(X, Yh)
    gen = torch.Generator().manual_seed(48)
    ever_reset, relief, delayed = torch.zeros(n, dtype=torch.bool), 0, 0
    for t in range(12):
        a = 0.3 * torch.randn(n, X.num_actions, generator=gen)
        X.step(a.to(device))
        copy_state(X, Yh)
        step = int(X._step_dev.item()) + 1000 * t  # any number: the same one for both
        X._native.post_physics(X.seed, step, X._stream())
        Yh._native.post_physics(Yh.seed, step, Yh._stream())
        bx, by = bound(X), bound(Yh)
        assert_equal(bx, by, ["reset", "episode_length", "sensor_count", "scan_delay", "scan_noise", "scan_dropout",
                              "scan_offset", "measured_heights"], f"step {t}")
        ever_reset |= X.reset_buf.cpu().bool()
        for name in ("scan", "scan_history"):
            g, h = bx[name].cpu(), by[name].cpu()
            assert torch.equal(g.view(torch.int32), h.view(torch.int32)), (name, t, float((g - h).abs().max()))
        mh = by["measured_heights"]
        relief += int(((mh.max(1).values - mh.min(1).values) > 1e-3).sum())
        delayed += int((by["sensor_count"].long() > 1).sum())
    assert bool(ever_reset.any()) and not bool(ever_reset.all())
    assert relief > 0 and delayed > 0
    assert int(X.sensor_count.max()) > K and int(X.sensor_count.min()) >= 1
    ids = torch.arange(0, n, 3, device=X.device)
    X.reset_idx(ids)  # lgx_reset_envs empties the rings of the envs it resets
    assert int(X.sensor_count[ids].abs().sum()) == 0 and int(X.sensor_count[1::3].min()) >= 1


# ------------------------------------------------------------------ 8. refusals and clamps
def refusals(device, tmp_path):
    import pytest
    from legged_gym_custom_amd import _native
    from legged_gym_custom_amd import params as prm
    from legged_gym_custom_amd.envs import task_registry_configs
    with pytest.raises(ValueError, match="LGX_MAX_SENSOR_HISTORY"):
        make_env("go2", 8, device, **{"domain_rand.max_scan_delay_s": capacity(5)})
    make_env("go2", 8, device, **{"domain_rand.max_scan_delay_s": capacity(4)})  # K = 4 is allowed
    both = make_env("go2", 8, device, **{"domain_rand.max_scan_delay_s": capacity(1), "domain_rand.max_obs_delay_s": capacity(3)})
    assert both.scan_history.shape[1] == 3 == both.sensor_history.shape[1] and both._scan_delay_cap == 1
    plain = make_env("go2", 8, device)
    S = plain.num_scan_obs
    with pytest.raises(ValueError, match="without scan latency"):
        plain.set_scan_delay(0.02)

    def refused(env, match, **attrs):
        for k, v in attrs.items():
            setattr(env, k, v)
        with pytest.raises(_native.LgxError, match=match):
            env._bind()
        for k in attrs:
            setattr(env, k, None)

    i32 = lambda *s: torch.zeros(*s, dtype=torch.int32, device=device)  # noqa: E731
    f32 = lambda *s: torch.zeros(*s, device=device)  # noqa: E731
    refused(plain, "scan_delay needs scan_history", scan_delay_steps=i32(8))
    refused(plain, "scan_delay needs scan_history", scan_delay_steps=i32(8), scan_history=f32(8, 1, S))  # no count
    refused(plain, "scan_delay needs scan_history", scan_delay_steps=i32(8), scan_history=f32(8, 1, S), sensor_count=i32(8))  # K = 0
    refused(plain, "scan_history needs sensor_count", scan_history=f32(8, 1, S))
    refused(plain, "scan_history with params.sensor_history_len = 0", scan_history=f32(8, 1, S), sensor_count=i32(8))
    refused(plain, "sensor_count needs sensor_history or scan_history", sensor_count=i32(8))
    plain._bind()
    # a task without a scan: the bind refuses every one of the five, the Python layer says why
    acfg = task_registry_configs("anymal_c_rough")[0]
    acfg.domain_rand.scan_model = True
    assert prm.scan_model(acfg, 0.02)["any"]
    noscan = make_env("anymal_c_rough", 8, device, tmp_path)  # the LEGGED task kind: no scan
    assert noscan.num_scan_obs == 0
    for name, t in (("scan_noise_amps", f32(8)), ("scan_dropouts", f32(8, 2)), ("scan_offsets", f32(8, 3)),
                    ("scan_delay_steps", i32(8)), ("scan_history", f32(8, 1, 1))):
        refused(noscan, "the scan model needs the Go2 task kind and params.num_scan > 0", **{name: t})
    noscan._bind()
    with pytest.raises(ValueError, match="no height scan"):
        noscan.set_scan_noise(0.1)
    with pytest.raises(ValueError, match="needs a task with a height scan"):
        make_env("anymal_c_rough", 8, device, tmp_path, **{"domain_rand.scan_model": True})
    # setters: a refused value writes nothing
    env = make_env("go2", 8, device, **{"domain_rand.max_scan_delay_s": capacity(2)})
    env.set_scan_delay(0.04)  # 2 control steps: the capacity
    for bad in (0.06, -0.02, float("nan"), torch.zeros(7)):
        with pytest.raises(ValueError):
            env.set_scan_delay(bad)
    assert int(env.scan_delay_steps.min()) == 2 == int(env.scan_delay_steps.max())
    env.set_scan_noise(0.05)
    for bad in (-0.1, float("inf"), float("nan"), torch.ones(7), torch.ones(8, 2)):
        with pytest.raises(ValueError):
            env.set_scan_noise(bad)
    assert float(env.scan_noise_amps.min()) == float(np.float32(0.05)) == float(env.scan_noise_amps.max())
    env.set_scan_dropout(0.25, 0.5)
    for bad in ((-0.1, 1.0), (1.5, 1.0), (0.1, 2.0), (float("nan"), 1.0), (torch.ones(7), 1.0), (0.1, float("nan"))):
        with pytest.raises(ValueError):
            env.set_scan_dropout(*bad)
    assert torch.equal(env.scan_dropouts.cpu(), torch.tensor([[0.25, 0.5]]).expand(8, 2))
    env.set_scan_offset(0.1, -0.1, 0.05)
    for bad in ((float("inf"), 0.0, 0.0), (0.0, torch.zeros(7), 0.0), (0.0, 0.0, float("nan"))):
        with pytest.raises(ValueError):
            env.set_scan_offset(*bad)
    assert torch.equal(env.scan_offsets.cpu(), torch.tensor([[0.1, -0.1, 0.05]]).expand(8, 3))
    # range errors of the config reader
    cfg = task_registry_configs("go2")[0]
    for key, bad in (("scan_noise_range", [-0.1, 0.1]), ("scan_noise_range", [0.2, 0.1]), ("scan_dropout_range", [0.0, 1.5]),
                     ("scan_offset_xy_range", [-0.1, 0.1]), ("scan_offset_z_range", [0.1, -0.1]),
                     ("scan_delay_range_s", [0.04, 0.02]), ("scan_dropout_value", 2.0), ("max_scan_delay_s", -1.0)):
        c = task_registry_configs("go2")[0]
        setattr(c.domain_rand, key, bad)
        with pytest.raises(ValueError):
            prm.scan_model(c, 0.02)
    c = task_registry_configs("go2")[0]
    c.domain_rand.randomize_scan_delay, c.domain_rand.scan_delay_range_s, c.domain_rand.max_scan_delay_s = True, [0.0, 0.06], 0.04
    with pytest.raises(ValueError, match="exceeds max_scan_delay_s"):
        prm.scan_model(c, 0.02)
    assert not prm.scan_model(cfg, 0.02)["any"]
    # the step clamps what the Python layer would refuse: a raw out-of-range tensor behaves as its clamp
    over = {"domain_rand.max_scan_delay_s": capacity(2)}
    raw, ref = make_env("go2_parkour", 8, device, **over), make_env("go2_parkour", 8, device, **over)
    ref.set_scan_delay(0.04)
    raw.scan_delay_steps.fill_(1 << 30)
    raw.scan_delay_steps[::2] = -5
    ref.scan_delay_steps[::2] = 0
    gen = torch.Generator().manual_seed(49)
    for e in (raw, ref):
        e.reset()
    for _ in range(5):
        a = torch.randn(8, raw.num_actions, generator=gen).to(device)
        raw.step(a.clone())
        ref.step(a.clone())
        assert_equal(bound(raw), bound(ref), ("root_states", "obs", "scan", "scan_history", "sensor_count"), "clamped delay")


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
    for call in (lambda: env.set_scan_noise(0.02), lambda: env.set_scan_dropout(0.1), lambda: env.set_scan_offset(0.1, 0.0)):
        with pytest.raises(RuntimeError, match="captured"):
            call()
    assert env.scan_noise_amps is None and env.scan_dropouts is None and env.scan_offsets is None


# ------------------------------------------------------------------ 10. the Python layer
RAND = {"domain_rand.randomize_scan_noise": True, "domain_rand.scan_noise_range": [0.0, 0.05],
        "domain_rand.randomize_scan_dropout": True, "domain_rand.scan_dropout_range": [0.0, 0.3],
        "domain_rand.randomize_scan_offset": True, "domain_rand.scan_offset_xy_range": [0.0, 0.1],
        "domain_rand.scan_offset_z_range": [-0.02, 0.02],
        "domain_rand.randomize_scan_delay": True, "domain_rand.scan_delay_range_s": [0.0, 0.04]}


def setup_draws(device, monkeypatch):
    n = 64
    base = {"domain_rand.randomize_kp_kd": True, "domain_rand.randomize_base_mass": True,
            "domain_rand.randomize_action_delay": True, "domain_rand.action_delay_range_s": [0.0, 0.03],
            "domain_rand.randomize_motor_strength": True,
            "domain_rand.randomize_obs_noise_scale": True, "domain_rand.obs_noise_scale_range": [0.5, 2.0],
            "domain_rand.randomize_obs_bias": True, "domain_rand.obs_bias_level_range": [0.0, 2.0],
            "domain_rand.randomize_obs_delay": True, "domain_rand.obs_delay_range_s": [0.0, 0.02],
            "domain_rand.randomize_external_force": True}
    X, Y = make_env("go2", n, device, **base, **RAND), make_env("go2", n, device, **base)
    for name in ("friction", "mass_params", "kp_kd", "action_delay", "motor_strength", "obs_noise_scale", "obs_bias",
                 "obs_delay", "force_window", "force_vec"):  # every earlier draw keeps its values
        assert torch.equal(bound(X)[name], bound(Y)[name]), name
    assert Y.scan_noise_amps is None and Y.scan_dropouts is None and Y.scan_offsets is None and Y.scan_history is None
    assert Y.sensor_history.shape[1] == 1 and X.sensor_history.shape[1] == 2  # max(0.02, 0.04) s of capacity
    S = X.num_scan_obs
    am, dr, of, dl = X.scan_noise_amps, X.scan_dropouts, X.scan_offsets, X.scan_delay_steps
    assert am.shape == (n,) and float(am.min()) >= 0.0 and float(am.max()) <= 0.05 and len(am.unique()) > n // 2
    assert float(dr[:, 0].min()) >= 0.0 and float(dr[:, 0].max()) <= 0.3 and float(dr[:, 1].min()) == 1.0 == float(dr[:, 1].max())
    r = of[:, :2].norm(dim=1)
    assert float(r.max()) <= 0.1 + 1e-6 and float(of[:, 0].min()) < 0 < float(of[:, 0].max()) and float(of[:, 1].min()) < 0
    assert float(of[:, 2].min()) >= -0.02 and float(of[:, 2].max()) <= 0.02
    assert dl.dtype == torch.int32 and int(dl.min()) >= 0 and int(dl.max()) <= 2 and len(dl.unique()) == 3
    assert X.scan_history.shape == (n, 2, S)
    import torch.distributed as dist
    for rank in (0, 1):  # two ranks of 32 envs draw rows [0, 32) and [32, 64) of the single-process draw
        monkeypatch.setattr(dist, "is_initialized", lambda: True)
        monkeypatch.setattr(dist, "get_rank", lambda group=None, rank=rank: rank)
        monkeypatch.setattr(dist, "get_world_size", lambda group=None: 2)
        Sx = make_env("go2", n // 2, device, **base, **RAND)
        monkeypatch.undo()
        sl = slice(rank * n // 2, (rank + 1) * n // 2)
        assert Sx.env_id_offset == rank * n // 2 and Sx.num_envs_total == n
        assert torch.equal(Sx.scan_noise_amps, am[sl]) and torch.equal(Sx.scan_dropouts, dr[sl])
        assert torch.equal(Sx.scan_offsets, of[sl]) and torch.equal(Sx.scan_delay_steps, dl[sl])
        assert torch.equal(Sx.obs_biases, X.obs_biases[sl]) and torch.equal(Sx.force_vec, X.force_vec[sl])


def evaluator(device):
    """tests/test_gpu_eval.py's setup (64 envs, a 10-step episode) with the scan test."""
    import pytest
    import eval_case as E
    from legged_gym_custom_amd.utils.evaluator import REPORT_KEYS, PolicyEvaluator

    def make(task="go2", **over):
        env, tcfg, args = E.make_env(task, 64, device, **{"env.episode_length_s": 0.19, **over})
        return PolicyEvaluator(env, E.make_runner(env, tcfg, args))

    on = {"domain_rand.scan_model": True, "domain_rand.max_scan_delay_s": 0.04}
    a, b, plain = make(**on), make(**on), make()
    env = a.env
    own_a = (0.01 * (torch.arange(64) % 3)).to(device)
    own_d = (torch.arange(64) % 3).to(torch.int32).to(device)
    own_o = (torch.arange(64 * 3).view(64, 3) % 5).float().to(device) * 1e-2
    env.set_scan_noise(own_a)
    env.scan_offsets.copy_(own_o)
    env.scan_delay_steps.copy_(own_d)
    own_p = env.scan_dropouts.clone()
    # one bin of neutral values: the per-env records of a plain run()
    plain.run()
    one = a.run_scan_test()
    assert one["delay_steps"] == [0] and one["noise_m"] == [0.0] and one["dropout"] == [0.0] and one["offset_x_m"] == [0.0]
    assert torch.equal(env.scan_eval_acc, plain.env.eval_acc) and torch.equal(env.scan_eval_status, plain.env.eval_status)
    assert set(REPORT_KEYS) == set(one["total"]) == set(one["bins"][0][0][0][0])
    for k in REPORT_KEYS:
        assert one["total"][k] == plain.report(plain.last_cells)["total"][k], k

    def own_back():
        assert torch.equal(env.scan_noise_amps, own_a) and torch.equal(env.scan_offsets, own_o)
        assert torch.equal(env.scan_delay_steps, own_d) and torch.equal(env.scan_dropouts, own_p)

    own_back()
    grid = dict(noise_m=(0.0, 0.05), dropout=(0.0, 0.3), offset_x_m=(-0.1, 0.1), delay_s=(0.0, 0.04))
    ra = a.run_scan_test(**grid)
    assert ra["graph"] is (device != "cpu") and ra["delay_steps"] == [0, 2] and ra["total"]["running"] == 0
    flat = [c for i in ra["bins"] for j in i for k in j for c in k]
    assert len(ra["bins"]) == 2 and len(flat) == 16
    sizes = [c["episodes"] + c["running"] for c in flat]
    assert sum(sizes) == 64 and max(sizes) - min(sizes) <= 1 and ra["total"]["episodes"] == 64
    cells = a.last_cells.clone()
    assert cells.shape == (4, 4, 12)
    rb = b.run_scan_test(graph=False, **grid)
    assert rb["graph"] is False and torch.equal(cells, b.last_cells)  # graph replay == the eager loop
    own_back()
    assert float(b.env.scan_noise_amps.abs().sum()) == 0.0 and float(b.env.scan_offsets.abs().sum()) == 0.0
    graph = a._scan_graph
    a.run_scan_test(noise_m=(0.01, 0.02), dropout=(0.1, 0.2), offset_x_m=(0.0, 0.05), delay_s=(0.02, 0.04))  # the same shape
    assert a._scan_graph is graph
    if device != "cpu":
        assert graph is not None
        a.run_scan_test(noise_m=(0.01,), dropout=(0.1, 0.2), offset_x_m=(0.0, 0.05), delay_s=(0.02, 0.04))
        assert a._scan_graph is not graph  # another shape: its own capture
        with pytest.raises(RuntimeError, match="captured"):
            plain.run_scan_test(noise_m=(0.0, 0.02))  # allocating now would re-bind under plain's captured loop
    rg = a.run_scan_test(gait=True, **grid)
    assert rg["bins"][1][1][1][1]["gait"]["envs"] == rg["bins"][1][1][1][1]["episodes"] and "gait" in rg["total"]
    for bad in (dict(noise_m=()), dict(dropout=[]), dict(offset_x_m=()), dict(delay_s=()), dict(noise_m=(-1.0,)),
                dict(dropout=(1.5,)), dict(offset_x_m=(float("nan"),)), dict(delay_s=(float("inf"),)), dict(delay_s=(0.06,))):
        with pytest.raises(ValueError):
            a.run_scan_test(**bad)
    with pytest.raises(ValueError):
        plain.run_scan_test(delay_s=(0.02,))  # no capacity
    own_back()


def evaluate_cli_document(device, tmp_path):
    """legged_gym/scripts/evaluate.py (a child process: it edits the registry's configs) on a checkpoint of
    randomly initialised networks: the scan test's document."""
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
                        "--scan_offset_m=-0.1,0,0.1", "--scan_delay_ms", "0,20", "--scan_noise_m", "0,0.02",
                        "--task=go2", f"--sim_device={device}", f"--rl_device={device}", "--num_envs=8", "--headless"],
                       cwd=str(tmp_path), env=penv, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    doc = json.loads(r.stdout.strip().splitlines()[-1])
    assert doc["task"] == "go2" and doc["policy"] == "student" and doc["num_steps"] == 3
    assert doc["noise_m"] == [0.0, 0.02] and doc["dropout"] == [0.0] and doc["offset_x_m"] == [-0.1, 0.0, 0.1]
    assert doc["delay_s"] == [0.0, 0.02] and doc["delay_steps"] == [0, 1] and doc["dropout_value"] == 1.0
    assert len(doc["bins"]) == 2 and all(len(p) == 1 and len(p[0]) == 3 and all(len(r) == 2 for r in p[0]) for p in doc["bins"])
    assert "episodes" in doc["bins"][1][0][2][1] and "total" in doc
    out = os.path.join(os.path.dirname(doc["checkpoint"]), "eval_student_scan.json")
    assert os.path.dirname(doc["checkpoint"]).startswith(str(tmp_path))
    with open(out) as f:
        assert json.load(f) == doc


def training_smoke(device, num_steps_per_env=None):
    import eval_case as E
    env, tcfg, args = E.make_env("go2", 64, device, **RAND)
    assert int(env.scan_delay_steps.max()) > 0 and float(env.scan_noise_amps.sum()) > 0
    if num_steps_per_env:
        tcfg.runner.num_steps_per_env = num_steps_per_env
    runner = E.make_runner(env, tcfg, args)
    runner.learn(num_learning_iterations=2, init_at_random_ep_len=True)
    if device != "cpu":
        assert env.graph_capturable and len(runner._graphs) > 0  # the rollout was captured and replayed
    assert torch.isfinite(env.obs_buf).all() and torch.isfinite(env.scan_obs_buf).all()
    assert torch.isfinite(env.scan_history).all() and float(env.scan_history.abs().sum()) > 0
    assert all(torch.isfinite(p).all() for p in runner.alg.actor_critic.parameters())
    ran = 2 * int(tcfg.runner.num_steps_per_env) + 1  # (+ the step reset() ends with)
    assert int(env.sensor_count.min()) >= 1 and int(env.sensor_count.max()) <= ran
    assert float(env.scan_obs_buf.abs().max()) <= 1.0
