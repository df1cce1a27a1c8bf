"""Worker of tests/test_gpu_ragged.py::test_ragged_sharding_through_rccl_at_world_size_1: ONE rank, backend nccl (= RCCL on ROCm), the
pattern of rccl_seam_world1_worker.py.  DSH_FORCE_COLLECTIVES=1 keeps the per-rank code paths from short-circuiting at world size 1, so
the ragged chains run where a multi-rank job runs them — on the rank's own run of segments, before the device-side gather — and the
result must equal the plain single-process call bit for bit, with and without the seam repair."""
import os
import sys

import torch
import torch.distributed as dist

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from diffsheg_amd.config import get_config  # noqa: E402
from diffsheg_amd.synthetic import make_inputs  # noqa: E402
from diffsheg_amd.trainer import DDPMTrainer, sampler_namespace  # noqa: E402
from util import gpu_model  # noqa: E402


def main():
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    torch.cuda.set_device(0)
    dist.init_process_group("nccl", device_id=torch.device("cuda:0"))
    assert dist.get_backend() == "nccl" and dist.get_world_size() == 1
    cfg = get_config("show")
    model = gpu_model("show", "fp32")
    tr = DDPMTrainer(sampler_namespace(cfg), model)
    N = 637                                     # three chains of 234 / 234 / 169 frames
    inp = make_inputs(cfg, 1, frames=N, seed=9)
    audio, hub, pid = inp["audio_emb"].cuda(), inp["pretrain_aud_feat"].cuda(), inp["person_id"].cuda()
    os.environ["DSH_FORCE_COLLECTIVES"] = "0"
    ref = tr.sample_arbitrary_len_sharded(audio, pid, {"pretrain_aud_feat": hub}, 3, seed=11, ragged=True)
    ref_rep = tr.sample_arbitrary_len_sharded(audio, pid, {"pretrain_aud_feat": hub}, 3, seed=11, ragged=True, seam_repair=True)
    os.environ["DSH_FORCE_COLLECTIVES"] = "1"
    out = tr.sample_arbitrary_len_sharded(audio, pid, {"pretrain_aud_feat": hub}, 3, seed=11, inputs_on_rank0_only=True, ragged=True)
    out_rep = tr.sample_arbitrary_len_sharded(audio, pid, {"pretrain_aud_feat": hub}, 3, seed=11, inputs_on_rank0_only=True, ragged=True,
                                              seam_repair=True)
    torch.cuda.synchronize()
    assert out is not None and tuple(out.shape) == (1, N, cfg.net_dim_pose)
    assert torch.equal(out, ref), float((out - ref).abs().max())
    assert torch.equal(out_rep, ref_rep) and not torch.equal(ref_rep, ref)
    dist.barrier()
    dist.destroy_process_group()
    print("RCCL_RAGGED_WORLD1_OK")


if __name__ == "__main__":
    main()
