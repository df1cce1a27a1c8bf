"""The DSH_* runtime switches (no GPU): csrc/switches.h is the one place that reads the environment, its table is what the library
enumerates through dsh_switch_count / dsh_switch_info, the tests and INTEGRATION.md section 4b name no switch the table does not have,
no GPU test flips a latched switch inside its own process, and the parsing quirks of the switches give the values the hand-written
expressions gave before the table existed (each expected value is quoted from the line that used to compute it)."""
import ast
import ctypes as C
import glob
import json
import os
import re
import subprocess
import sys

import pytest

from diffsheg_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "diffsheg_amd", "csrc")
TOKEN = re.compile(r"\bDSH_[A-Z0-9_]+\b")
PROCESS, CONTEXT, CALL = 0, 1, 2

# variables that Python code reads itself (never the library)
PYTHON_VARIABLES = {
    "DSH_PIN",                    # diffsheg_amd/hostenv.py: NUMA pinning of a rank
    "DSH_FORCE_COLLECTIVES",      # diffsheg_amd/trainer.py: run the collectives at world size 1
    "DSH_BENCH_DRYRUN",           # bench.py: rendezvous + timing contract only
    "DSH_BENCH_OVERSUBSCRIBE",    # bench.py: several ranks on one GPU
    "DSH_BENCH_BACKEND",          # bench.py: collective backend
    "DSH_BENCH_ZERO_DATA",        # bench.py: power probe
}
# DSH_* tokens of the Python files that are not environment variables
NOT_VARIABLES = {
    "DSH_LAUNCH_COUNT_ENTRIES",   # C macro of include/diffsheg_hip.h: entries of dsh_debug_launch_counts
    "DSH_METRICS_HEADER",         # C macro of include/diffsheg_hip.h: header words of the batch-metrics result
    "DSH_NOISE_STACK",            # C enum value of include/diffsheg_hip.h: dsh_sampler_opts.noise_mode
}


def _table():
    L = _lib.lib()
    name, default, help_ = C.c_char_p(), C.c_char_p(), C.c_char_p()
    when, cls = C.c_int32(), C.c_int32()
    rows = {}
    for i in range(L.dsh_switch_count()):
        kind = _lib.check(L.dsh_switch_info(i, C.byref(name), C.byref(default), C.byref(when), C.byref(cls), C.byref(help_)))
        rows[name.value.decode()] = {"kind": kind, "default": default.value.decode(), "when": when.value, "cls": cls.value, "help": help_.value.decode()}
    return rows


TABLE = _table()


def test_the_table_is_well_formed_and_refuses_what_it_does_not_have():
    L = _lib.lib()
    assert L.dsh_switch_count() == len(TABLE) == 47               # (no duplicate names)
    for name, row in TABLE.items():
        assert TOKEN.fullmatch(name) and row["kind"] in (0, 1, 2) and row["when"] in (PROCESS, CONTEXT, CALL) and row["cls"] in (0, 1, 2, 3), (name, row)
        assert row["default"] and len(row["help"]) > 10, name
    assert L.dsh_switch_info(-1, None, None, None, None, None) == -1 and L.dsh_switch_info(len(TABLE), None, None, None, None, None) == -1
    assert L.dsh_switch_info(0, None, None, None, None, None) == 0            # every output pointer may be null
    assert L.dsh_switch_read(b"NOT_A_SWITCH", None, None) == -1 and L.dsh_switch_read(None, None, None) == -1
    assert b"NOT_A_SWITCH" not in L.dsh_last_error() and b"dsh_switch_read" in L.dsh_last_error()


def test_one_file_reads_the_environment_and_it_reads_the_table():
    readers = [f for f in sorted(glob.glob(os.path.join(CSRC, "*"))) if os.path.isfile(f) and "getenv" in open(f, errors="replace").read()]
    assert [os.path.basename(f) for f in readers] == ["switches.h"]
    assert set(re.findall(r'"(DSH_[A-Z0-9_]+)"', open(readers[0]).read())) == set(TABLE)


def test_python_names_no_switch_the_table_does_not_have():
    files = glob.glob(os.path.join(ROOT, "tests", "*.py")) + glob.glob(os.path.join(ROOT, "diffsheg_amd", "*.py")) + \
        [os.path.join(ROOT, "bench.py"), os.path.join(ROOT, "__graft_entry__.py")]
    assert not (PYTHON_VARIABLES | NOT_VARIABLES) & set(TABLE)
    for f in files:
        unknown = set(TOKEN.findall(open(f).read())) - set(TABLE) - PYTHON_VARIABLES - NOT_VARIABLES
        assert not unknown, (os.path.relpath(f, ROOT), sorted(unknown))


def _environ(node):
    return isinstance(node, ast.Attribute) and node.attr == "environ"


def _env_writes(tree):
    """(function, key node) of every write to the process's own environment: monkeypatch.setenv / os.putenv, os.environ[k] = ...,
    os.environ.update / setdefault.  `function` is the enclosing top-level def (None at module level)."""
    found = []
    for top in tree.body:
        fn = top if isinstance(top, (ast.FunctionDef, ast.AsyncFunctionDef)) else None
        for n in ast.walk(top):
            if isinstance(n, ast.Call) and isinstance(n.func, ast.Attribute):
                if n.func.attr in ("setenv", "putenv") and n.args:
                    found.append((fn, n.args[0]))
                elif n.func.attr in ("update", "setdefault") and _environ(n.func.value):
                    found += [(fn, ast.Constant(k.arg)) for k in n.keywords if k.arg]
                    for a in n.args[:1]:
                        found += [(fn, k) for k in a.keys] if isinstance(a, ast.Dict) else [(fn, a)]
            elif isinstance(n, (ast.Assign, ast.AugAssign)):
                for t in (n.targets if isinstance(n, ast.Assign) else [n.target]):
                    if isinstance(t, ast.Subscript) and _environ(t.value):
                        found.append((fn, t.slice))
    return found


def test_no_gpu_test_flips_a_latched_switch_in_its_own_process():
    """A PROCESS switch is latched by its first read, so a test that flips one with monkeypatch.setenv / os.environ compares an arm
    with itself and passes whatever the other arm does.  Such a switch goes into the env= of a fresh worker process.  A key that is
    not a literal stands for every DSH_* literal of its test function, decorators included."""
    latched = {n for n, r in TABLE.items() if r["when"] == PROCESS}
    assert {"DSH_GP_DMA", "DSH_GEMM_KSPLIT", "DSH_AUD_HOIST", "DSH_PIPE_ROWS", "DSH_GRAPH_ROWS"} <= latched
    files = sorted(glob.glob(os.path.join(ROOT, "tests", "test_gpu_*.py")))
    assert files
    for f in files:
        src = open(f).read()
        for fn, key in _env_writes(ast.parse(src)):
            if isinstance(key, ast.Constant):
                names = {key.value} if isinstance(key.value, str) else set()
            else:
                names = set(TOKEN.findall(ast.get_source_segment(src, fn) or "")) if fn else set(TOKEN.findall(src))
                for d in (fn.decorator_list if fn else []):
                    names |= set(TOKEN.findall(ast.get_source_segment(src, d) or ""))
            assert not names & latched, (os.path.basename(f), getattr(fn, "name", None), sorted(names & latched))


def test_the_scanner_of_environment_writes_sees_every_form():
    src = ('import os\n'
           'import pytest\n'
           '@pytest.mark.parametrize("k", ["VAR_A", "VAR_B"])\n'
           'def t(k, monkeypatch):\n'
           '    monkeypatch.setenv(k, "0")\n'
           '    monkeypatch.setenv("VAR_C", "0")\n'
           '    os.environ["VAR_D"] = "1"\n'
           '    os.environ.update(VAR_E="1")\n'
           '    os.environ.setdefault("VAR_F", "1")\n'
           '    run(env=dict(os.environ, VAR_G="1"))\n')
    keys = [k.value if isinstance(k, ast.Constant) else "<expr>" for _, k in _env_writes(ast.parse(src))]
    assert sorted(keys) == ["<expr>", "VAR_C", "VAR_D", "VAR_E", "VAR_F"]


def test_integration_guide_lists_the_table():
    md = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    sec = md[md.index("## 4b."):]
    sec = sec[:sec.index("\n## ", 4)]
    rows = [ln for ln in sec.splitlines() if ln.startswith("| `DSH_")]
    first_col = set()
    for ln in rows:
        cells = re.split(r"(?<!\\)\|", ln)
        first_col |= set(TOKEN.findall(cells[1]))
        assert re.search(r"PROCESS|CONTEXT|CALL|Python", cells[2]), ln          # the column that says when the switch is read
    assert first_col == set(TABLE) | PYTHON_VARIABLES, sorted(first_col ^ (set(TABLE) | PYTHON_VARIABLES))
    assert set(TOKEN.findall(sec)) <= set(TABLE) | PYTHON_VARIABLES
    when_word = {PROCESS: "PROCESS", CONTEXT: "CONTEXT", CALL: "CALL"}
    for ln in rows:                                                            # a row's column names the `when` of each of its switches
        cells = re.split(r"(?<!\\)\|", ln)
        for name in TOKEN.findall(cells[1]):
            assert ("Python" if name in PYTHON_VARIABLES else when_word[TABLE[name]["when"]]) in cells[2], (name, cells[2])
    assert "fresh process" in sec


def _reads(*words):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "switch_read_worker.py"), *words], capture_output=True, text=True, timeout=60,
                       env={k: v for k, v in os.environ.items() if not k.startswith("DSH_")})
    assert r.returncode == 0, r.stderr[-2000:]
    return [tuple(x[1:]) for x in json.loads(r.stdout.strip().splitlines()[-1])]


# (what is set, what is read, [(is_set, value)] expected) — is_set is 0 for a derivation.  Behind each row: the expression that computed
# the value before the table existed (file:line of the last commit without csrc/switches.h).
UNSET, DERIVED = 0, 0
KNOWN = [
    # denoiser.hip:1316  nsplit_ = e ? std::max(1, std::min(8, atoi(e) == 1 ? 2 : atoi(e))) : 3;
    # denoiser.hip:1317  if (e && atoi(e) == 0) nsplit_ = 1;
    ([], ["DSH_DUAL", "dual_streams"], [(UNSET, 3), (DERIVED, 3)]),
    (["DSH_DUAL=0"], ["DSH_DUAL", "dual_streams"], [(1, 0), (DERIVED, 1)]),
    (["DSH_DUAL=1"], ["dual_streams"], [(DERIVED, 2)]),
    (["DSH_DUAL=5"], ["dual_streams"], [(DERIVED, 5)]),
    (["DSH_DUAL=99"], ["DSH_DUAL", "dual_streams"], [(1, 99), (DERIVED, 8)]),
    (["DSH_DUAL=-4"], ["dual_streams"], [(DERIVED, 1)]),
    # denoiser.hip:40  sw.ffn_ver = (fv && atoi(fv) == 2) ? 2 : 3;      capi.hip:605 and profiler.h:44: the same test
    ([], ["DSH_FFN_V", "ffn_generation"], [(UNSET, 3), (DERIVED, 3)]),
    (["DSH_FFN_V=2"], ["ffn_generation"], [(DERIVED, 2)]),
    (["DSH_FFN_V=3"], ["ffn_generation"], [(DERIVED, 3)]),
    (["DSH_FFN_V=7"], ["DSH_FFN_V", "ffn_generation"], [(1, 7), (DERIVED, 3)]),
    # tl2.hip:1037  const bool roll_on = !(roll_e && atoi(roll_e) == 0);      -> the empty string switches a default-on switch OFF
    ([], ["DSH_TL2_ROLL"], [(UNSET, 1)]),
    (["DSH_TL2_ROLL="], ["DSH_TL2_ROLL"], [(1, 0)]),
    (["DSH_TL2_ROLL=on"], ["DSH_TL2_ROLL"], [(1, 0)]),
    # denoiser.hip:1763  for (k : {"DSH_PIPE", "DSH_LEVEL_PREFETCH", "DSH_LEVEL_CACHE"}) { v = getenv(k); if (v && atoi(v) == 0) return false; }
    ([], ["pipe_switches_on"], [(DERIVED, 1)]),
    (["DSH_PIPE="], ["pipe_switches_on"], [(DERIVED, 0)]),
    (["DSH_LEVEL_PREFETCH=0"], ["pipe_switches_on"], [(DERIVED, 0)]),
    (["DSH_LEVEL_CACHE=0"], ["pipe_switches_on"], [(DERIVED, 0)]),
    (["DSH_PIPE=2", "DSH_LEVEL_CACHE=1"], ["pipe_switches_on"], [(DERIVED, 1)]),
    # sampler.hip:401  ... && getenv("DSH_NO_GRAPH") == nullptr;      -> presence only: =0 is present, so graphs are off
    ([], ["DSH_NO_GRAPH"], [(UNSET, 0)]),
    (["DSH_NO_GRAPH=0"], ["DSH_NO_GRAPH"], [(1, 0)]),
    # denoiser.hip:58  if (tr && atoi(tr) > 0) sw.tls_rows = atoi(tr);      :1326, :1328 the same for DSH_DUAL_ROWS / DSH_DUAL_MIN_ROWS
    (["DSH_TLS_ROWS=-1"], ["DSH_TLS_ROWS", "tls_rows_override"], [(1, -1), (DERIVED, 0)]),
    (["DSH_TLS_ROWS=3000"], ["tls_rows_override"], [(DERIVED, 3000)]),
    (["DSH_TLS_ROWS=0"], ["tls_rows_override"], [(DERIVED, 0)]),
    # denoiser.hip:65  sw.f32_bits = (fp32 && latent_dim == 512) ? (f3 ? atoi(f3) & 15 : 15) : 0;
    ([], ["f32_fuse_bits"], [(DERIVED, 15)]),
    (["DSH_F32_FUSE=31"], ["DSH_F32_FUSE", "f32_fuse_bits"], [(1, 31), (DERIVED, 15)]),
    (["DSH_F32_FUSE=4"], ["f32_fuse_bits"], [(DERIVED, 4)]),
    # denoiser.hip:44  sw.hilo = ... && !(hl && atoi(hl) == 0);      capi.hip:486, :510, :633  he && atoi(he) != 0
    ([], ["hilo_denoiser", "hilo_op"], [(DERIVED, 1), (DERIVED, 0)]),
    (["DSH_HILO=0"], ["hilo_denoiser", "hilo_op"], [(DERIVED, 0), (DERIVED, 0)]),
    (["DSH_HILO=1"], ["hilo_denoiser", "hilo_op"], [(DERIVED, 1), (DERIVED, 1)]),
    (["DSH_HILO="], ["hilo_denoiser", "hilo_op"], [(DERIVED, 0), (DERIVED, 0)]),
    # tl3_ffn.hip:752  pc = pc_e ? std::min(2, std::max(0, atoi(pc_e))) : 1;      :756  pb_e ? (atoi(pb_e) & 3) : 1
    # denoiser.hip:1130  return (!e || (atoi(e) & 1)) && (!pc || atoi(pc) == 1);      (e: DSH_FFN_PB, pc: DSH_FFN_PC)
    ([], ["ffn_pc", "ffn_pb", "ffn_keeps_hi_plane"], [(DERIVED, 1), (DERIVED, 1), (DERIVED, 1)]),
    (["DSH_FFN_PC=9", "DSH_FFN_PB=7"], ["ffn_pc", "ffn_pb", "ffn_keeps_hi_plane"], [(DERIVED, 2), (DERIVED, 3), (DERIVED, 0)]),
    (["DSH_FFN_PC=-3", "DSH_FFN_PB=2"], ["ffn_pc", "ffn_pb", "ffn_keeps_hi_plane"], [(DERIVED, 0), (DERIVED, 2), (DERIVED, 0)]),
    # gemm.hip:527 and denoiser.hip:69  e ? atoi(e) : 512      sampler.hip:413 and denoiser.hip:1330  e ? (size_t)atol(e) : 64499
    # sampler.hip:463 and denoiser.hip:1319  l ? atoi(l) : 3      sampler.hip:399  e ? (size_t)atol(e) : 4096
    ([], ["gemm_ksplit_rows", "gemm_ksplit_rows_context", "pipe_rows", "pipe_rows_context", "DSH_DUAL_LAG", "DSH_GRAPH_ROWS"],
     [(DERIVED, 512), (DERIVED, 512), (DERIVED, 64499), (DERIVED, 64499), (UNSET, 3), (UNSET, 4096)]),
    (["DSH_GEMM_KSPLIT=0", "DSH_PIPE_ROWS=100"], ["gemm_ksplit_rows", "gemm_ksplit_rows_context", "pipe_rows", "pipe_rows_context"],
     [(DERIVED, 0), (DERIVED, 0), (DERIVED, 100), (DERIVED, 100)]),
]


@pytest.mark.parametrize("case", range(len(KNOWN)))
def test_parsing_quirks_give_the_values_the_old_expressions_gave(case):
    setup, reads, want = KNOWN[case]
    assert _reads(*setup, *reads) == want, (setup, reads)


def test_a_latched_switch_keeps_its_first_value_and_a_per_call_switch_follows_the_environment():
    assert TABLE["DSH_GP_DMA"]["when"] == PROCESS and TABLE["DSH_PIPE"]["when"] == CALL and TABLE["DSH_GEMM_KSPLIT"]["when"] == PROCESS
    # gemm_f32_pro.hip:588  static const int dma_on = [] { const char* e = getenv("DSH_GP_DMA"); return e ? atoi(e) : 1; }();
    assert _reads("DSH_GP_DMA=0", "DSH_GP_DMA", "DSH_GP_DMA=1", "DSH_GP_DMA", "-DSH_GP_DMA", "DSH_GP_DMA") == [(1, 0), (1, 0), (1, 0)]
    assert _reads("DSH_GP_DMA", "DSH_GP_DMA=0", "DSH_GP_DMA") == [(0, 1), (0, 1)]            # latched while unset: stays unset
    # denoiser.hip:1541  const char* off = getenv("DSH_PIPE");      (in pipe_begin: every loop looks again)
    assert _reads("DSH_PIPE=0", "DSH_PIPE", "DSH_PIPE=1", "DSH_PIPE", "-DSH_PIPE", "DSH_PIPE") == [(1, 0), (1, 1), (0, 1)]
    # DSH_GEMM_KSPLIT has both: gemm.hip:527 latches it (static const int ks_rows), denoiser.hip:69 reads it per context
    assert _reads("DSH_GEMM_KSPLIT=0", "gemm_ksplit_rows", "DSH_GEMM_KSPLIT=64", "gemm_ksplit_rows", "gemm_ksplit_rows_context") == \
        [(0, 0), (0, 0), (0, 64)]
    # a latched string outlives the environment it was read from (tl2.hip:951: DSH_STAGGER is parsed once)
    assert _reads("DSH_STAGGER=4,100,3", "DSH_STAGGER", "-DSH_STAGGER", "DSH_STAGGER") == [(1, 4), (1, 4)]
