"""`python legged_gym/scripts/evaluate.py --task=go2` — batched policy evaluation with
per-terrain metrics, running legged_gym_custom_amd.scripts.evaluate."""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

from legged_gym_custom_amd.scripts.evaluate import main  # noqa: E402

if __name__ == "__main__":
    main()
