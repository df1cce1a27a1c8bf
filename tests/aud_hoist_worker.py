"""Worker of tests/test_gpu_eval.py::test_aud_hoist_agrees_with_the_front_recomputed_in_every_evaluation: one bf16
evaluation of the test's batch with DSH_AUD_HOIST as the environment gives it, eps written to argv[1].  The switch is latched by the first
read in a process (PROCESS in csrc/switches.h), so the arm that differs from the test process's own value needs a fresh process."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import torch  # noqa: E402

from diffsheg_amd.config import get_config  # noqa: E402
from util import HOIST_CASE, eval_call, gpu_model, hoist_latched  # noqa: E402

cfg = get_config("show")
eps = eval_call(gpu_model("show", "bf16"), cfg, HOIST_CASE.inputs(cfg), *HOIST_CASE.args).cpu()
assert hoist_latched() == int(int(os.environ["DSH_AUD_HOIST"]) != 0), "the library did not read the worker's DSH_AUD_HOIST"
torch.save(eps, sys.argv[1])
print("AUD_HOIST_WORKER_OK", os.environ["DSH_AUD_HOIST"])
