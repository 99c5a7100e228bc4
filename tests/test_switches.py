"""csrc/switches.hpp is the one list of the engine's MI_* environment switches.  These checks read source text only (no device, no
built library): every switch name the engine, DESIGN.md's appendix or a test spells is a name of that list, with the list's default."""
import fnmatch
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "rapidcfd-dev_amd", "csrc")
ROW = re.compile(r'^\s*X\((\w+),\s*("MI_[A-Z0-9_]+"|nullptr),\s*(-?\d+),\s*([A-Z| ]+?),\s*(USER|AB|TRANSPORT|DIAG),\s*("\w+"|nullptr),\s*"(.+)"\)\s*\\?$', re.M)
WHEN = {"ONCE", "CTX", "ADDR", "ROWS", "HIER", "ATTACH", "PERSIST", "CALL"}
# the reads that the hashed part of gamg_engine.inc (tools/source_fingerprint.py) keeps spelling with their defaults
HASHED_READS = {"MI_PEER_ALLOW_COARSE", "MI_GAMG_REG_INVERT", "MI_GAMG_INVERT_OVERLAP", "MI_GAMG_INVERT_V2"}
NOT_SWITCHES = set()   # "MI_..." string literals in csrc/ that are no environment names: none today


def _read(*path):
    with open(os.path.join(*path)) as f:
        return f.read()


def _table():
    """environment name (or option name, for a row without one) -> (default, when, group, option)"""
    rows = ROW.findall(_read(CSRC, "switches.hpp"))
    t = {(env.strip('"') if env != "nullptr" else opt.strip('"')): (int(d), set(w.replace(" ", "").split("|")), grp, None if opt == "nullptr" else opt.strip('"'))
         for _, env, d, w, grp, opt, _ in rows}
    assert len(t) == len(rows) and len(rows) == _read(CSRC, "switches.hpp").count("\n    X("), "a row of the table did not parse, or a name is there twice"
    return t


def _sources():
    return {os.path.basename(p): _read(p) for p in sorted(glob.glob(os.path.join(CSRC, "*"))) if os.path.basename(p) != "switches.hpp"}


def _appendix():
    """the four engine groups of DESIGN.md's appendix (name -> default as written), and the Python-side names of its last paragraph"""
    text = _read(ROOT, "DESIGN.md").split("## Appendix: switches", 1)[1]
    engine, python = text.split("Python side", 1)
    rows = dict(re.findall(r"^\| `(MI_[A-Z0-9_]+)` \| (-?\d+) \|", engine, re.M))
    in_rows = "\n".join(line for line in engine.splitlines() if line.startswith("|"))
    return rows, set(re.findall(r"\b(MI_[A-Z0-9_]+)", in_rows)), set(re.findall(r"`(MI_[A-Z0-9_*]+)`", python))


def test_table_rows_are_well_formed():
    t = _table()
    assert len(t) >= 60
    for name, (_, when, _, option) in t.items():
        assert when and when <= WHEN, name
        assert option is None or "CTX" in when, f"{name}: mi_ctx_set_option stores into a context member"
    assert sorted(o for _, _, _, o in t.values() if o) == ["fuse_prologue", "gamg_graph_attached", "pcg_fuse_rp", "pcg_fuse_test", "pcg_persist", "win_direct"]
    assert "pcg_fuse_test" in t, "the option without an environment name"


def test_every_name_in_csrc_is_in_the_table():
    t = _table()
    for fname, text in _sources().items():
        for name in re.findall(r'"(MI_[A-Z0-9_]+)"', text):
            assert name in t or name in NOT_SWITCHES, f"{fname}: {name} is not in csrc/switches.hpp"


def test_reads_outside_the_table_are_the_four_hashed_ones():
    t = _table()
    found = []
    for fname, text in _sources().items():
        assert 'getenv("MI_' not in text, fname
        assert not re.search(r'env_int_host\s*\(', text), fname
        found += [(fname, n, int(d)) for n, d in re.findall(r'env_int\s*\(\s*"(MI_[A-Z0-9_]+)"\s*,\s*(-?\d+)\s*\)', text)]
        assert len(re.findall(r'env_int\s*\([^)]*"MI_', text)) == sum(1 for f, _, _ in found if f == fname), f"{fname}: an env_int read this test cannot parse"
    assert sorted(n for _, n, _ in found) == sorted(HASHED_READS) and {f for f, _, _ in found} == {"gamg_engine.inc"}, found
    for _, name, dflt in found:
        assert dflt == t[name][0], f"{name}: gamg_engine.inc says {dflt}, the table {t[name][0]}"


def test_design_appendix_is_the_table():
    t = _table()
    rows, engine_names, _ = _appendix()
    for name, (dflt, _, _, option) in t.items():
        if name == option:
            continue   # no environment name
        assert name in rows, f"{name} is missing from DESIGN.md's appendix"
        assert int(rows[name]) == dflt, f"{name}: DESIGN.md says {rows[name]}, the table {dflt}"
    assert engine_names <= set(t), sorted(engine_names - set(t))


def test_every_name_a_test_sets_is_known():
    """every quoted "MI_..." literal in tests/*.py (however it reaches setenv: directly, through a dict or a loop variable) and every
    MI_...= keyword (dict(...), _Env(...)) is a switch of the table or a Python-side name of the appendix"""
    t = _table()
    _, _, python_side = _appendix()
    quoted = re.compile(r"""["'](MI_[A-Z0-9_]+)["']""")
    keyword = re.compile(r"\b(MI_[A-Z0-9_]+)=(?!=)")
    n = 0
    for path in sorted(glob.glob(os.path.join(ROOT, "tests", "*.py"))):
        if os.path.basename(path) == "test_switches.py":
            continue
        text = _read(path)
        for name in quoted.findall(text) + keyword.findall(text):
            n += 1
            assert name in t or any(fnmatch.fnmatchcase(name, p) for p in python_side), f"{os.path.basename(path)}: {name} is neither in csrc/switches.hpp nor a Python-side name of DESIGN.md's appendix"
    assert n > 100   # (the patterns still find the tests' settings)


# rows of group USER or AB that no test sets to another value than the default, and why
EXEMPT = {
    "MI_HOST_THP": "read once per process (ONCE) and host allocation only: the tables hold the same values either way",
    "MI_PCG_FUSE_COOP": "read once per process (ONCE): a test of it needs a process of its own",
}


def _values_given(text, name, option):
    """what a test file gives a switch: the literal integers where the text has one ("MI_X", "0" / MI_X="0" / MI_X=0 /
    set_option("opt", 0)), None where the value is an expression; an environment name that is only deleted does not count"""
    found = []
    pats = [r"""(?<!delenv\()["']%s["']\s*[,:]?\s*(?:str\()?["']?(-?\d+)?""" % name, r"""\b%s=(?!=)["']?(-?\d+)?""" % name]
    if option:
        pats.append(r"""set_option\(\s*["']%s["']\s*,\s*(-?\d+)?""" % option)
    for pat in pats:
        found += [int(v) if v else None for v in re.findall(pat, text)]
    return found


def test_every_same_bits_switch_is_exercised():
    """every USER or AB row is given a value other than its default by some file under tests/ (by its environment name, quoted or
    as a keyword, or by its option name in a set_option call), or stands in EXEMPT with the reason: a form that "gives the same
    results either way" is a claim the suite has to run.  TRANSPORT and DIAG rows need several devices or inject faults."""
    t = _table()
    texts = {os.path.basename(p): _read(p) for p in sorted(glob.glob(os.path.join(ROOT, "tests", "*.py"))) if os.path.basename(p) != "test_switches.py"}
    missing = []
    for name, (dflt, _, group, option) in t.items():
        if group not in ("USER", "AB"):
            continue
        given = [v for text in texts.values() for v in _values_given(text, name, option)]
        exercised = any(v is None or v != dflt for v in given)
        assert not (exercised and name in EXEMPT), f"{name} is exercised: take it out of EXEMPT"
        if not exercised and name not in EXEMPT:
            missing.append(name)
    assert not missing, f"no test sets {missing} to another value than the default"
    assert set(EXEMPT) <= set(t)
