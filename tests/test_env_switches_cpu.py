"""The library's environment switches: one table (csrc/smm_env.h), one getenv, one list ("Environment switches"),
and the accessors themselves under AddressSanitizer + UBSan (tests/cpp/env_case.cpp, built by tests/cpp/Makefile)."""
import glob
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "sparse_matrix_math_amd", "csrc")
ROW = re.compile(r'\bX\(\s*(\w+)\s*,\s*"(\w+)"\s*,\s*(ONCE|EACH)\s*,\s*(SPEED|ARITH|TRANSPORT|DIAG|LAB)\s*,\s*"((?:[^"\\]|\\.)+)"\s*\)')
NAME = r"(?:SMM_HIP_[A-Z0-9_]+|SMM_RESIDENT_LAB)"


def registry():
    """{variable: policy} from the X-macro rows of smm_env.h"""
    with open(os.path.join(CSRC, "smm_env.h")) as f:
        rows = ROW.findall(f.read())
    names = [r[1] for r in rows]
    assert len(rows) >= 60 and len(set(names)) == len(names) and len({r[0] for r in rows}) == len(rows), "rows not parsed, or a name twice"
    assert all(re.fullmatch(NAME, n) for n in names), names
    return {r[1]: r[2] for r in rows}


def sources():
    return sorted(glob.glob(os.path.join(CSRC, "*.hip")) + glob.glob(os.path.join(CSRC, "*.h")))


def strip_comments(text):
    """C++ source without // and /* */ comments (string and character literals are kept whole)"""
    out, i, n = [], 0, len(text)
    while i < n:
        c = text[i]
        if c in "\"'":
            j = i + 1
            while j < n and text[j] != c:
                j += 2 if text[j] == "\\" else 1
            out.append(text[i:j + 1])
            i = j + 1
        elif text.startswith("//", i):
            while i < n and text[i] != "\n":
                i += 1
        elif text.startswith("/*", i):
            i = text.index("*/", i) + 2
            out.append(" ")
        else:
            out.append(c)
            i += 1
    return "".join(out)


def test_strip_comments_keeps_code_and_literals():
    src = 'a = getenv("X//y"); // getenv("Z")\n/* getenv("W") */ b = \'"\'; c = "q\\"//r";\n'
    assert strip_comments(src) == 'a = getenv("X//y"); \n  b = \'"\'; c = "q\\"//r";\n'


def test_the_document_lists_the_registry():
    reg = registry()
    with open(os.path.join(ROOT, "INTEGRATION.md")) as f:
        text = f.read()
    section = text.split("## Environment switches", 1)[1].split("\n## ", 1)[0]
    table = section.split("Two more are read by the Python binding", 1)[0]  # (those two are not the library's)
    listed = {}
    for line in table.splitlines():
        cells = [c.strip() for c in line.strip().strip("|").split("|")]
        m = re.fullmatch("`(" + NAME + ")`", cells[0]) if len(cells) == 5 else None
        if m:
            assert m.group(1) not in listed, m.group(1)
            assert cells[2] in ("once per process", "every create / call"), line
            assert cells[1] and cells[3] and cells[4], line
            listed[m.group(1)] = "ONCE" if cells[2] == "once per process" else "EACH"
    assert set(listed) == set(reg), sorted(set(listed) ^ set(reg))
    assert listed == reg, sorted(n for n in reg if listed[n] != reg[n])
    for extra in ("SMM_HIP_LIBRARY", "SMM_HIP_SYSTEM_RUNTIME"):  # read by _lib.py
        assert extra not in reg and "`" + extra + "`" in section


def test_getenv_is_called_in_one_header_only():
    callers = []
    for path in sources():
        with open(path) as f:
            if re.search(r"\bgetenv\s*\(", strip_comments(f.read())):
                callers.append(os.path.basename(path))
    assert callers == ["smm_env.h"]


def test_no_switch_is_named_by_a_string_outside_the_table():
    """the accessors take identifiers; a variable's name as a string literal of its own exists in the table's rows only"""
    reg = registry()
    for path in sources():
        with open(path) as f:
            literals = re.findall('"(' + NAME + ')"', strip_comments(f.read()))
        if os.path.basename(path) == "smm_env.h":
            assert sorted(literals) == sorted(reg)
        else:
            assert literals == [], (os.path.basename(path), literals)


def test_accessors_under_address_and_ub_sanitizers():
    """unset / numbers / empty and non-numeric text / flags / EACH follows, ONCE keeps -- run directly, nothing preloaded"""
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "tests", "cpp"), "env_case"], check=True)
    env = {k: v for k, v in os.environ.items() if not re.fullmatch(NAME, k)}
    r = subprocess.run([os.path.join(ROOT, "tests", "cpp", "env_case")], capture_output=True, text=True, timeout=60, env=env)
    assert r.returncode == 0 and " 0 failed" in r.stdout, r.stdout[-3000:] + r.stderr[-3000:]
    assert "runtime error" not in r.stderr and "Sanitizer" not in r.stderr, r.stderr[-3000:]
