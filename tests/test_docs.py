"""The documents the review reads are kept in the shape it asked for: DESIGN.md is a current-state
document of at most 400 lines with one byte table, one kernel table, one parity, one measurement and one multi-GPU
section; the round-by-round narrative lives in HISTORY.md; profiles/README.md indexes the evidence newest round first;
every profile file the current-state documents cite exists."""
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _read(name):
    with open(os.path.join(ROOT, name)) as f:
        return f.read()


def test_design_is_a_current_state_document():
    d = _read("DESIGN.md")
    assert d.count("\n") <= 400
    for heading in ("## 1. The path and its boundary", "## 2. Data layout in HBM", "## 3. The fused KKT step",
                    "### Algorithmic bytes per iteration", "## 4. Kernels", "## 5. Parity", "## 6. Measurement",
                    "## 7. Multi-GPU", "## 8. Out of scope"):
        assert d.count(heading) == 1, heading
    assert "@" not in re.sub(r"`[^`]*`", "", d).replace("@k", ""), "an unfilled placeholder of tools/dbg/DESIGN.md.in"
    assert "HISTORY.md" in d and os.path.exists(os.path.join(ROOT, "HISTORY.md"))


def test_profiles_readme_is_newest_first():
    r = _read("profiles/README.md")
    pos = [r.index("# round %d evidence" % k) for k in (6, 5, 4, 3, 2, 1)]
    assert pos == sorted(pos)


def test_cited_profile_files_exist():
    cited = set()
    for doc in ("DESIGN.md", "README.md"):
        cited |= set(re.findall(r"profiles/(r0[0-9]_[A-Za-z0-9_.]+\.(?:jsonl|json|csv|txt))", _read(doc)))
    assert cited, "the documents cite their evidence"
    missing = sorted(f for f in cited if not os.path.exists(os.path.join(ROOT, "profiles", f)))
    assert not missing, missing


def test_switch_table_is_the_only_registry():
    """Every environment switch of the library is one entry of the table in context.cpp, each entry is a row of the
    INTEGRATION.md switch table and the other way round, and no other code reads a PAROPT_AMD_ variable (besides the
    table's reader only PAROPT_AMD_RCCL_LIB, a path, is read directly)."""
    csrc = os.path.join(ROOT, "paropt_amd", "csrc")
    table = set(re.findall(r'\{SW_\w+, "(PAROPT_AMD_\w+)"', _read("paropt_amd/csrc/context.cpp")))
    documented = set(re.findall(r"^\| \d+ \| `(PAROPT_AMD_\w+)`", _read("INTEGRATION.md"), re.M))
    assert table and table == documented, (sorted(table - documented), sorted(documented - table))
    direct = []
    for f in sorted(os.listdir(csrc)):
        if f.endswith((".cpp", ".hpp", ".hip")):
            direct += [(f, v) for v in re.findall(r'getenv\("(PAROPT_AMD_\w+)"', _read(os.path.join("paropt_amd", "csrc", f)))]
    assert direct == [("context.cpp", "PAROPT_AMD_RCCL_LIB")], direct
    # tools/ab_switch.py resets every id between its variants
    count = re.search(r"SW_COUNT = (\d+)", _read("paropt_amd/csrc/core.hpp")).group(1)
    assert re.search(r"^SW_COUNT = %s\b" % count, _read("tools/ab_switch.py"), re.M), count
