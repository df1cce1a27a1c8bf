"""Worker of tests/test_switches_cpu.py: replays argv in a fresh process (so nothing is latched yet) against the library's own reading
of the DSH_* switches.  "NAME=VALUE" sets a variable, "-NAME" unsets it, any other word is read through dsh_switch_read (a switch of
the table, or one of the derivations of csrc/switches.h).  Prints one JSON list of [word, is_set, value] per read.  No GPU."""
import ctypes as C
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from diffsheg_amd import _lib  # noqa: E402

L = _lib.lib()
out = []
for word in sys.argv[1:]:
    if "=" in word:
        k, v = word.split("=", 1)
        os.environ[k] = v
    elif word.startswith("-"):
        os.environ.pop(word[1:], None)
    else:
        is_set, value = C.c_int32(-1), C.c_int64(-1)
        _lib.check(L.dsh_switch_read(word.encode(), C.byref(is_set), C.byref(value)), word)
        out.append([word, is_set.value, value.value])
print(json.dumps(out))
