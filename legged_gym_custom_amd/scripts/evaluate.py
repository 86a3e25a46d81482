"""evaluate.py — how good is the trained policy: the latest checkpoint of the task's experiment
(loaded as play.py loads it) is run for one episode in every env, on the device, and survival,
command tracking and cost of transport are reported per terrain level x type
(legged_gym_custom_amd/utils/evaluator.py). The terrain and command curricula are switched off
(every env keeps its tile; the command ranges are the configured ones); the rest of the config
stays as trained: observation noise, pushes, friction / mass / gain randomisation.

  python legged_gym/scripts/evaluate.py --task=go2_parkour --num_envs=4096 [--policy student|teacher]
         [--eval_steps N]

One JSON document is printed and written next to the checkpoint (eval_<policy>.json)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import isaacgym  # noqa: E402,F401  (placeholder, as in play.py)
import torch  # noqa: E402

from legged_gym_custom_amd import LEGGED_GYM_ROOT_DIR  # noqa: E402
from legged_gym.envs import *  # noqa: E402,F401,F403
from legged_gym.utils import get_args, get_load_path, task_registry  # noqa: E402
from legged_gym_custom_amd.utils.evaluator import PolicyEvaluator  # noqa: E402


def evaluate(args, policy="student", eval_steps=None, root=None, graph=True):
    env_cfg, train_cfg = task_registry.get_cfgs(name=args.task)
    env_cfg.terrain.curriculum = False
    env_cfg.commands.curriculum = False
    env, _ = task_registry.make_env(name=args.task, args=args, env_cfg=env_cfg)

    train_cfg.runner.resume = True
    log_root = os.path.join(os.environ.get("LGX_LOG_ROOT") or os.path.join(root or LEGGED_GYM_ROOT_DIR, "logs"),
                            train_cfg.runner.experiment_name)
    runner, train_cfg = task_registry.make_alg_runner(env=env, name=args.task, args=args, train_cfg=train_cfg,
                                                      log_root=log_root)
    checkpoint = get_load_path(log_root, load_run=train_cfg.runner.load_run, checkpoint=train_cfg.runner.checkpoint)
    report = PolicyEvaluator(env, runner, policy=policy).run(eval_steps, graph=graph)
    report = dict(task=args.task, checkpoint=checkpoint, iteration=int(runner.current_learning_iteration), **report)
    out = os.path.join(os.path.dirname(checkpoint), f"eval_{policy}.json")
    with open(out, "w") as f:
        json.dump(report, f, indent=1)
    return report, out


def main(argv=None):
    p = argparse.ArgumentParser(add_help=False)
    p.add_argument("--policy", choices=("student", "teacher"), default="student")
    p.add_argument("--eval_steps", type=int, default=None)
    own, rest = p.parse_known_args(sys.argv[1:] if argv is None else argv)
    torch.set_float32_matmul_precision("high")
    report, _ = evaluate(get_args(rest), policy=own.policy, eval_steps=own.eval_steps)
    print(json.dumps(report))
    return report


if __name__ == "__main__":
    main()
