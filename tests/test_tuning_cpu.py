"""CPU: the tuning table stays honest.

* every knob the library reads (a `tune_on / tune_is / tune_int / tune_has("NAME"` call under csrc/) is a row of the table in INTEGRATION.md
  section 6 and the other way round; the two debug knobs of `-DSEFD_TUNING` builds are named in that section's prose instead;
* no reader keeps a value (no `static` initialised from the table) and the string read serves `sefd_tuning_get` alone;
* `clear()` returns to the pairs of the environment variable SEFD_TUNING (an empty table without it);
* a planner knob set after a first plan was built reaches the next plan."""
import importlib.util
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dnn-based-speech-enhancement-in-the-frequency-domain_amd", "csrc")
DEBUG_BUILD_KNOBS = {"CG256_DBG", "WG_DBG"}            # read inside #ifdef SEFD_TUNING only


def _sources():
    for f in sorted(os.listdir(CSRC)):
        if f.endswith((".hip", ".cpp", ".h")):
            with open(os.path.join(CSRC, f)) as fh:
                yield f, fh.read().splitlines()


def _section6():
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    start = text.index("\n## 6. Tuning table")
    end = text.find("\n## ", start + 1)
    return text[start:end if end > 0 else len(text)]


def test_knobs_read_equal_knobs_documented():
    read, by_variable = set(), []
    for f, lines in _sources():
        if f in ("tuning.cpp", "tuning.h"):
            continue
        for n, line in enumerate(lines, 1):
            code = line.split("//")[0]
            for m in re.finditer(r"\btune_(?:on|is|int|has|str)\(\s*([^,)]*)", code):
                arg = m.group(1).strip()
                lit = re.fullmatch(r'"([A-Z0-9_]+)"', arg)
                if lit:
                    read.add(lit.group(1))
                elif not (f == "api.hip" and "sefd_tuning_get" in code):
                    by_variable.append(f"{f}:{n}: {line.strip()}")
    assert not by_variable, "knob names must be spelled at the call site:\n" + "\n".join(by_variable)
    sec = _section6()
    table = set()
    for line in sec.splitlines():
        if line.startswith("| `"):
            table.update(re.findall(r"`([A-Z][A-Z0-9_]+)`", line.split("|")[1]))
    assert len(table) > 30, table
    for k in DEBUG_BUILD_KNOBS:
        assert k in read and k not in table and f"`{k}`" in sec, k
    assert read - DEBUG_BUILD_KNOBS == table, (sorted(read - DEBUG_BUILD_KNOBS - table), sorted(table - read))


def test_no_latched_knob_and_one_string_reader():
    latched, strs = [], []
    for f, lines in _sources():
        for n, line in enumerate(lines, 1):
            if re.search(r"static .*tune_", line):
                latched.append(f"{f}:{n}: {line.strip()}")
            if "tune_str(" in line and f not in ("tuning.cpp", "tuning.h") and "sefd_tuning_get" not in line:
                strs.append(f"{f}:{n}: {line.strip()}")
            if f != "tuning.cpp" and re.search(r"ato(i|ll)\(tune_", line):
                strs.append(f"{f}:{n}: {line.strip()}")
    assert not latched, "\n".join(latched)
    assert not strs, "\n".join(strs)


_CHILD = r"""
import sys
sys.path.insert(0, sys.argv[1])
import sefd_amd
from sefd_amd import tuning
assert tuning.get("CG256_MINM") == "64", tuning.get("CG256_MINM")
tuning.set("CG256_MINM", 128)
assert tuning.get("CG256_MINM") == "128"
tuning.set("BN_FUSE", 2)
with tuning.scope(NO_OVERLAP=None):
    assert tuning.get("NO_OVERLAP") is None
tuning.clear()
assert tuning.get("CG256_MINM") == "64", tuning.get("CG256_MINM")
assert tuning.get("NO_OVERLAP") == "1", tuning.get("NO_OVERLAP")
assert tuning.get("BN_FUSE") is None
tuning.unset("CG256_MINM")
assert tuning.get("CG256_MINM") is None
tuning.clear()
assert tuning.get("CG256_MINM") == "64"
print("child ok")
"""


def test_clear_returns_to_the_environment_table():
    # a fresh process: the variable is parsed once, the first time the table is consulted
    env = dict(os.environ, SEFD_TUNING="CG256_MINM=64,NO_OVERLAP=1")
    r = subprocess.run([sys.executable, "-c", _CHILD, ROOT], env=env, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "child ok" in r.stdout, r.stdout + r.stderr


def test_clear_without_the_variable_leaves_an_empty_table():
    assert "SEFD_TUNING" not in os.environ
    import sefd_amd  # noqa: F401
    from sefd_amd import tuning
    tuning.set("CG256_MINM", 64)
    tuning.set("NO_OVERLAP", 1)
    tuning.clear()
    for k in ("CG256_MINM", "NO_OVERLAP", "BN_FUSE"):
        assert tuning.get(k) is None, k


def test_planner_knob_set_after_a_first_plan_reaches_the_next_plan():
    """The chunked LSTM forward of the knob arms' plan (its layer-1 input GEMMs on the third lane: what the removed LSTM_LANE3 latch chose once per
    process) is planned first; LSTM_CHUNKS=1 set afterwards must give the plan the fingerprint matrix records for it, and the default comes back."""
    spec = importlib.util.spec_from_file_location("plan_fingerprint", os.path.join(ROOT, "tools", "plan_fingerprint.py"))
    fp = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(fp)
    import sefd_amd  # noqa: F401
    from sefd_amd import tuning
    want = {}
    for line in open(os.path.join(ROOT, "profiles", "tuning_refactor_fingerprints.txt")):
        if not line.startswith("#"):
            name, parent, head = line.split()
            assert parent == head, name
            want[name] = head
    assert want["arm_LSTM_CHUNKS=1"] != want["arm_base"] != want["arm_LANE_ALL=0"]
    base = fp.digest(fp.plan_bytes(fp.ARM, {}))
    assert base == want["arm_base"]
    with tuning.scope(LSTM_CHUNKS=1):
        assert fp.digest(fp.plan_bytes(fp.ARM, {})) == want["arm_LSTM_CHUNKS=1"]
    assert fp.digest(fp.plan_bytes(fp.ARM, {})) == base
    tuning.set("LANE_ALL", 0)
    assert fp.digest(fp.plan_bytes(fp.ARM, {})) == want["arm_LANE_ALL=0"]
    tuning.clear()
    assert fp.digest(fp.plan_bytes(fp.ARM, {})) == base
