"""dsh_run_spec on the host (the library only, no GPU): dsh_sample_count against the counting entries of the compatibility layer over
the grids of test_editing_cpu.py and test_fewstep_cpu.py, every refusal a spec can earn without a context with the message fragment
of the old path, and the struct_size rule (a shorter struct reads its missing tail as zero, a longer one is refused)."""
import ctypes as C

import pytest

import fewstep_ref as F
from diffsheg_amd import _lib
from diffsheg_amd.diffusion import space_timesteps

STRIDE10 = sorted(space_timesteps(1000, "ddim10"))


def _opts(resp, kind=0, jl=3, jn=5, eta=0.0, son=0):
    return _lib.SamplerOptsC(kind, 1000, resp, jl, jn, 10, 1, 0, 0, 0, 1, 0, son, 0, eta)


def _count(o, spec):
    """(rc, draws, steps, message) of dsh_sample_count"""
    lib = _lib.lib()
    d, s = C.c_int64(-7), C.c_int64(-7)
    rc = lib.dsh_sample_count(C.byref(o), C.byref(spec), C.byref(d), C.byref(s))
    return rc, d.value, s.value, lib.dsh_last_error()


def _old(o, masked, init, K, kept):
    lib = _lib.lib()
    arr = (C.c_int32 * max(len(kept), 1))(*kept)
    return (lib.dsh_sample_num_draws_subset(C.byref(o), masked, init, K, arr, len(kept)),
            lib.dsh_sample_num_steps_subset(C.byref(o), masked, init, K, arr, len(kept)))


GRID = [(0, 25, [], (3, 5)), (0, 25, [], (2, 3)), (0, 10, [], (3, 5)), (0, 10, STRIDE10, (3, 5)), (0, 10, F.LOGSNR10, (3, 5)), (1, 1, [], (3, 5))]


@pytest.mark.parametrize("masked", [0, 1])
@pytest.mark.parametrize("init", [0, 1, 2])
def test_count_equals_the_counting_entries(masked, init):
    n_ok = n_refused = 0
    for kind, resp, kept, (jl, jn) in GRID:
        o = _opts(resp, kind, jl, jn)
        for K in range(-1, resp + 2):
            want = _old(o, masked, init, K, kept)
            rc, draws, steps, _ = _count(o, _lib.run_spec(timesteps=kept, init=init, masked=masked, start_level=K))
            # (the draws entry refuses everything a spec is refused for; the steps entry never looked at init 2 on a DDPM loop)
            assert (rc == -1) == (want[0] == -1), (kind, resp, kept[:3], K, rc, want)
            if rc == 0:
                assert (draws, steps) == want, (kind, resp, kept[:3], K, draws, steps, want)
                n_ok += 1
            else:
                n_refused += 1
    assert n_ok > 0 and n_refused > 0
    # the figures test_editing_cpu.py and test_fewstep_cpu.py pin, through the new entry
    if init == 0:
        assert _count(_opts(25), _lib.run_spec(masked=masked))[1:3] == ((175, 111) if masked else (26, 25))
        assert _count(_opts(10), _lib.run_spec(timesteps=F.LOGSNR10, masked=masked))[1:3] == ((1 + 2 * 31 + 24, 55) if masked else (11, 10))


def test_reverse_specs_count_their_levels_and_no_draws():
    for kept, resp in (([], 25), (F.LOGSNR10, 10)):
        assert _count(_opts(resp), _lib.run_spec(timesteps=kept, invert_to=4))[:3] == (0, 0, 4)
        assert _count(_opts(resp), _lib.run_spec(timesteps=kept, invert_from=1, invert_to=resp, init=2, solver=1))[:3] == (0, 0, resp - 1)
    # either output may be null
    o, spec, s = _opts(25), _lib.run_spec(), C.c_int64()
    assert _lib.lib().dsh_sample_count(C.byref(o), C.byref(spec), None, C.byref(s)) == 0 and s.value == 25
    assert _lib.lib().dsh_sample_count(C.byref(o), C.byref(spec), None, None) == 0


def test_bad_specs_are_refused_with_the_old_message():
    lib = _lib.lib()
    ten = _opts(10)
    bad = [(ten, dict(timesteps=F.LOGSNR10[:9]), b"respacing"),                          # wrong subset length
           (ten, dict(timesteps=F.LOGSNR10[:-1] + [1000]), b"outside"),                  # subset entry >= steps
           (ten, dict(timesteps=[5, 5] + F.LOGSNR10[2:]), b"ascending"),
           (_opts(10, kind=1), dict(timesteps=F.LOGSNR10), b"DDIM"),                     # subset on DDPM
           (_opts(25, kind=1), dict(start_level=5), b"DDIM"),                            # start level on DDPM
           (_opts(25, kind=1), dict(init=2), b"DDIM loops only"),                        # init 2 on DDPM
           (_opts(25), dict(init=3), b"init"),
           (_opts(25), dict(invert_to=4, masked=1), b"mask"),                            # reverse with a mask
           (_opts(25), dict(invert_from=4, invert_to=4), b"from_level < to_level"),      # from_level >= to_level
           (_opts(25), dict(invert_from=5, invert_to=4), b"from_level < to_level"),
           (_opts(25), dict(invert_to=26), b"respacing"),
           (_opts(25), dict(invert_to=4, start_level=3), b"start level"),
           (_opts(25, eta=0.5), dict(invert_to=4), b"eta"),
           (_opts(25), dict(solver=2), b"solver"),                                       # unknown solver
           (_opts(25, eta=0.5), dict(solver=1), b"eta"),                                 # dpm2m with eta != 0
           (_opts(25, son=1), dict(solver=1), b"same_overlap_noisy"),
           (_opts(25, kind=1), dict(solver=1), b"DDIM loops only"),
           (_opts(25), dict(tail_blend=1, start_level=3), b"tail blend"),
           (_opts(25, son=1), dict(tail_blend=1), b"same_overlap_noisy"),
           (_opts(25), dict(row_keys=[1, 2]), None)]                                     # (keys alone are fine: their count is the run's to check)
    for o, fields, frag in bad:
        rc, d, s, msg = _count(o, _lib.run_spec(**fields))
        if frag is None:
            assert rc == 0, (fields, msg)
            continue
        assert rc == -1 and frag in msg, (fields, rc, msg)
        assert (d, s) == (-7, -7), "a refused count wrote its outputs"
    # the same refusals through the counting entries the specs replace, where one exists: the same fragment
    for o, kept, K, init, frag in ((ten, F.LOGSNR10[:9], 0, 0, b"respacing"), (ten, F.LOGSNR10[:-1] + [1000], 0, 0, b"outside"),
                                   (_opts(10, kind=1), F.LOGSNR10, 0, 0, b"DDIM"), (_opts(25, kind=1), [], 5, 0, b"DDIM"),
                                   (_opts(25, kind=1), [], 0, 2, b"DDIM loops only")):
        assert _old(o, 0, init, K, kept)[0] == -1 and frag in lib.dsh_last_error(), (kept[:3], K, init)
    # null arguments
    o, spec = _opts(25), _lib.run_spec()
    assert lib.dsh_sample_count(None, C.byref(spec), None, None) == -1 and lib.dsh_sample_count(C.byref(o), None, None, None) == -1


def test_struct_size_rule():
    lib = _lib.lib()
    o = _opts(10)
    full = C.sizeof(_lib.RunSpecC)
    assert _lib.RunSpecC.solver.offset + C.sizeof(C.c_int32) <= full                     # `solver` is the last field
    want = _count(o, _lib.run_spec(timesteps=F.LOGSNR10, masked=1, start_level=4))[:3]
    assert want[0] == 0 and want[1] > 0
    spec = _lib.run_spec(timesteps=F.LOGSNR10, masked=1, start_level=4, solver=7)
    rc, _, _, msg = _count(o, spec)
    assert rc == -1 and b"solver" in msg
    # one field short: the missing tail reads as zero, whatever the caller's memory holds there
    spec.struct_size = _lib.RunSpecC.solver.offset
    assert _count(o, spec)[:3] == want
    # shorter still: n_rows, the row pointers, tail_blend and the timestep list are gone as well -> the stride
    spec.struct_size = _lib.RunSpecC.timesteps.offset
    assert _count(o, spec)[:3] == _count(o, _lib.run_spec(masked=1, start_level=4))[:3]
    # larger than the library knows, and too small to hold struct_size itself
    for size in (full + 4, full + 8, 1 << 20, 0, 3):
        spec.struct_size = size
        rc, d, s, msg = _count(o, spec)
        assert rc == -1 and b"struct_size" in msg and (d, s) == (-7, -7), size
    spec.struct_size = full
    spec.solver = 0
    assert _count(o, spec)[:3] == want
