"""CPU tests (-m "not gpu") of the host side: C-ABI exports, native table/schedule code vs the golden
vectors, weight naming, window/shard logic, and that the product path refuses to run without a GPU."""
import ctypes as C
import json
import os
import re

import numpy as np
import pytest
import torch

from diffsheg_amd import _lib
from diffsheg_amd.config import get_config
from diffsheg_amd.diffusion import diffusion_table, get_schedule_jump_cjm_ddim, space_timesteps
from diffsheg_amd.trainer import get_windows, shard_range, split_segments
from diffsheg_amd.weights import make_synthetic_state_dict, state_dict_spec, validate_state_dict
from util import GOLDEN, golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_library_exports_every_declared_symbol():
    hdr = open(os.path.join(ROOT, "include", "diffsheg_hip.h")).read()
    declared = set(re.findall(r"\b(dsh_[a-z0-9_]+)\s*\(", hdr))
    assert declared, "no declarations parsed"
    lib = _lib.lib()                      # binds every name in _lib.SYMBOLS or raises
    assert declared == set(_lib.SYMBOLS), declared ^ set(_lib.SYMBOLS)
    for name in declared:
        assert hasattr(lib, name)
    assert b"gfx950" in lib.dsh_version()


def test_launch_counters_match_the_header_and_reset():
    """dsh_debug_launch_counts: the binding's names cover exactly the entries the header documents, a short buffer is not overrun,
    and a reset zeroes every entry (host-side counters: no GPU needed)."""
    import ctypes as C
    hdr = open(os.path.join(ROOT, "include", "diffsheg_hip.h")).read()
    n_hdr = int(re.search(r"#define DSH_LAUNCH_COUNT_ENTRIES (\d+)", hdr).group(1))
    assert n_hdr == len(_lib.LAUNCH_FAMILIES)
    for i, name in [(0, "tl_linear"), (5, "tl_small"), (6, "fused FFN"), (12, "gemm_f32_pro")]:
        assert re.search(rf"\b{i} {re.escape(name)}", hdr), (i, name)
    lib = _lib.lib()
    assert lib.dsh_debug_launch_counts(None, 0, 1) == n_hdr
    short = (C.c_int64 * 4)(7, 7, 7, 7)
    assert lib.dsh_debug_launch_counts(short, 2, 0) == n_hdr
    assert list(short) == [0, 0, 7, 7]
    assert set(_lib.launch_counts().values()) == {0}


def test_native_tables_match_reference_goldens():
    full, sp = golden("tables_ddpm1000.npz"), golden("tables_ddim25.npz")
    for k in full.files:
        np.testing.assert_allclose(diffusion_table(1000, 0, k), full[k], rtol=1e-15, atol=0, err_msg=k)
    for k in sp.files:
        if k != "timestep_map":
            np.testing.assert_allclose(diffusion_table(1000, 25, k), sp[k], rtol=1e-14, atol=0, err_msg=k)
    assert space_timesteps(1000, "ddim25") == set(int(v) for v in sp["timestep_map"])
    with pytest.raises(_lib.DshError):
        space_timesteps(1000, "ddim999")        # no integer stride gives exactly 999 steps (respace.py:30-32)


def test_native_jump_schedule_matches_reference_goldens():
    ref = json.load(open(os.path.join(GOLDEN, "schedules.json")))
    for key, want in ref.items():
        if key.startswith("resp20"):
            assert get_schedule_jump_cjm_ddim(20, 3, 5) == want
        else:
            jl, jn = (int(v) for v in key.split(","))
            assert get_schedule_jump_cjm_ddim(25, jl, jn) == want, key


def test_draw_and_step_counts():
    lib = _lib.lib()
    def opts(kind=0, jl=3, jn=5, no_repaint=0):
        return _lib.SamplerOptsC(kind, 1000, 25, jl, jn, 10, 1, 0, no_repaint, 0, 0, 0)
    o = opts()
    assert lib.dsh_sample_num_draws(C.byref(o), 0, 0) == 26
    assert lib.dsh_sample_num_draws(C.byref(o), 1, 0) == 1 + 63 * 2 + 48 == 175
    assert lib.dsh_sample_num_steps(C.byref(o), 1) == 111
    assert lib.dsh_sample_num_draws(C.byref(o), 0, 1) == 25
    o = opts(no_repaint=1)
    assert lib.dsh_sample_num_draws(C.byref(o), 1, 0) == 1 + 25 * 2
    o = opts(kind=1)
    assert lib.dsh_sample_num_draws(C.byref(o), 0, 0) == 1001


def test_state_dict_spec_counts():
    for ds, n_entries, n_params in [("show", 554, 155_779_775), ("beat", 552, 155_416_560)]:   # SURVEY §0 [probed]
        cfg = get_config(ds)
        spec = state_dict_spec(cfg)
        assert len(spec) == n_entries
        learnable = sum(int(np.prod(s)) for k, s, kind in spec
                        if kind not in ("pe", "counter", "bn_mean", "bn_var"))
        assert learnable == n_params


def test_validate_state_dict_errors():
    cfg = get_config("beat")
    sd = make_synthetic_state_dict(cfg, 1)
    validate_state_dict(cfg, sd)
    bad = dict(sd); bad.pop("encoder_ges.out.weight")
    with pytest.raises(KeyError):
        validate_state_dict(cfg, bad)
    bad = dict(sd); bad["time_embed.0.weight"] = torch.zeros(3, 3)
    with pytest.raises(ValueError):
        validate_state_dict(cfg, bad)


def test_get_windows_matches_reference_semantics():
    x = torch.arange(244).view(1, 244, 1)
    w = get_windows(x, 88, 78)
    assert [t.shape[1] for t in w] == [88, 88, 88] and int(w[2][0, 0, 0]) == 156
    w = get_windows(torch.zeros(1, 186, 2), 88, 78)
    assert [t.shape[1] for t in w] == [88, 88, 30]
    assert len(get_windows(torch.zeros(1, 50, 2), 88, 78)) == 1
    d = get_windows({"a": torch.zeros(1, 186, 2), "b": torch.zeros(1, 186, 3)}, 88, 78)
    assert len(d) == 3 and d[2]["b"].shape == (1, 30, 3)
    # 5-minute SHOW audio: 9000 frames -> 116 windows, 30-frame tail
    w = get_windows(torch.zeros(1, 9000, 1), 88, 78)
    assert len(w) == 116 and w[-1].shape[1] == 30


def test_window_chain_masks_and_fix_very_first():
    """Chain bookkeeping of sample_arbitrary_len against the oracle's window_chain (ddpm_show_trainer.py:864-906),
    with a stand-in for generate_batch: the out-paint mask / gt hand-off, the tail window and --fix_very_first."""
    import argparse
    from diffsheg_amd.trainer import DDPMTrainer
    from oracle import sampler_ref as S
    C_, L, n_poses, N = 6, 10, 88, 186
    torch.manual_seed(0)
    audio, hub, motions = torch.randn(2, N, 4), torch.randn(2, N, 3), torch.randn(2, N, C_)

    def fake_window(i, a, h, y):              # deterministic function of everything the sampler receives
        base = a.sum(-1, keepdim=True) + h.sum(-1, keepdim=True) + 0.01 * i
        out = base.expand(-1, -1, C_).clone()
        if y:
            out = torch.where(y["outpainting_mask"], y["gt"], out)
        return out

    class Stub(DDPMTrainer):
        def __init__(self, opt):
            self.opt, self.device, self.calls = opt, torch.device("cpu"), 0
        def generate_batch(self, a, p_id, dim_pose, add_cond={}, inpaint_dict=None, **kw):
            self.calls += 1
            return fake_window(self.calls - 1, a, add_cond["pretrain_aud_feat"], inpaint_dict)

    for fix in (False, True):
        opt = argparse.Namespace(n_poses=n_poses, overlap_len=L, net_dim_pose=C_, fix_very_first=fix)
        tr = Stub(opt)
        got = tr.sample_arbitrary_len(audio, torch.zeros(2, 4), {"pretrain_aud_feat": hub}, motions=motions if fix else None)
        ref = S.window_chain(fake_window, audio, hub, n_poses, L, C_, fix_very_first_motions=motions if fix else None)
        assert tr.calls == 3 and got.shape == (2, N, C_)
        assert torch.equal(got, ref)
        if fix:
            assert torch.equal(got[:, :L], motions[:, n_poses - L:n_poses])
    with pytest.raises(ValueError):
        Stub(argparse.Namespace(n_poses=n_poses, overlap_len=L, net_dim_pose=C_, fix_very_first=True)).sample_arbitrary_len(
            audio, torch.zeros(2, 4), {"pretrain_aud_feat": hub})


def test_shard_and_segment_partition():
    for n, world in [(950, 8), (7, 8), (2500, 8), (116, 3)]:
        parts = [shard_range(n, r, world) for r in range(world)]
        flat = [i for p in parts for i in p]
        assert flat == list(range(n))
        assert max(len(p) for p in parts) - min(len(p) for p in parts) <= 1
    segs = split_segments(9000, 8, 88, 10)
    assert segs[0].start == 0 and segs[-1].stop == 9000
    assert all(a.stop == b.start for a, b in zip(segs[:-1], segs[1:]))
    assert all(len(s) > 10 for s in segs)


def test_product_path_fails_loudly_without_gpu():
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from diffsheg_amd.model import UniDiffuser
    with pytest.raises(_lib.DshError):
        UniDiffuser(get_config("beat"), {}, device="cuda:0")


def test_product_modules_never_import_oracle():
    pkg = os.path.join(ROOT, "diffsheg_amd")
    for fn in os.listdir(pkg):
        if fn.endswith(".py"):
            src = open(os.path.join(pkg, fn)).read()
            assert "import oracle" not in src and "from oracle" not in src, fn


def test_window_seed_has_no_small_integer_collisions():
    """Philox key of (seed, window): a hash, so that neighbouring seeds / windows never share a stream (round 2 used seed + window,
    and XORed the chain id into it: (s + 1) ^ 0 == s ^ 1)."""
    from diffsheg_amd.trainer import window_seed
    keys = {window_seed(s, w) for s in range(2000, 2064) for w in range(64)}
    assert len(keys) == 64 * 64
    assert all(0 <= k < 2 ** 64 for k in keys)
    assert window_seed(11, 0) != window_seed(11, 1) != window_seed(12, 0)
    assert window_seed(2 ** 64 + 5, 3) == window_seed(5, 3)          # seeds are taken modulo 2^64, like the C ABI's uint64


def test_kernel_build_id_covers_every_source_and_the_compile_flags():
    """Every file that holds a kernel (__global__), every header, the host files that pick grids / instantiations and the
    Makefile (compile flags) are part of the build id (round-3 advisor finding: a hand-kept list missed them)."""
    import glob
    from diffsheg_amd import buildid
    hashed = {os.path.basename(f) for f in buildid.kernel_sources()}
    assert all(os.path.exists(f) for f in buildid.kernel_sources())
    for f in glob.glob(os.path.join(buildid._CSRC, "*")):
        if f.endswith((".hip", ".h")):
            assert os.path.basename(f) in hashed, f
    assert {"Makefile", "denoiser.hip", "capi.hip", "diffsheg_hip.h"} <= hashed
    assert len(buildid.kernel_build_id()) == 16


def test_denoiser_interfaces_are_all_pure_and_the_one_base_is_gone():
    """csrc/denoiser.h declares two interfaces, DenoiserInstance (one model on one stream) and DenoiserContext (what a dsh_ctx owns).
    Neither carries a method whose body means "not supported on this kind of object": every virtual other than a destructor is pure,
    and the type that once united the two roles, with the class that implemented the context's half of it, is named nowhere in the sources."""
    import glob
    csrc = os.path.join(ROOT, "diffsheg_amd", "csrc")
    hdr = open(os.path.join(csrc, "denoiser.h")).read()
    code = re.sub(r"//[^\n]*", "", hdr)                                       # (declarations only: comments mention `virtual` too)
    decls = re.findall(r"\bvirtual\b[^;{]*[;{]", code)
    assert len(decls) > 40, len(decls)
    for d in decls:
        if re.search(r"\bvirtual\s+~", d):
            continue
        assert re.search(r"=\s*0\s*;$", d), f"virtual with a default body: {' '.join(d.split())}"
    for name in ("DenoiserInstance", "DenoiserContext"):
        assert re.search(rf"\bclass {name} \{{", code), name
    for f in glob.glob(os.path.join(csrc, "*")):
        if os.path.isfile(f):
            text = open(f, errors="replace").read()
            assert "DenoiserBase" not in text and "DualDenoiser" not in text, f
