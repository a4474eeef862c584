"""build()'s unit table is the one list of the library's translation units: it names every *.hip of csrc/ (HOST_UNITS every *.cpp), and the variant build keeps no
list of its own (it once did, and a variant library then lacked the unit the list had not caught up with)."""
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry      # noqa: E402

CSRC = os.path.join(ROOT, "uv-slam_amd", "csrc")


def _includes(path, seen=None):
    """The csrc headers a source reaches through its #include "..." lines."""
    seen = set() if seen is None else seen
    with open(path) as f:
        for name in re.findall(r'^\s*#\s*include\s+"([^"/]+)"', f.read(), re.M):
            if name not in seen and os.path.exists(os.path.join(CSRC, name)):
                seen.add(name); _includes(os.path.join(CSRC, name), seen)
    return seen


# what a variant varies: every unit built from the persistent kernel's header or from the blob layout, and the packing that feeds them
REBUILT_BY_VARIANT = {row[0] for row in entry.UNITS if {"uvs_solve_kernel.h", "uvs_layout.h"} & _includes(os.path.join(CSRC, row[0] + ".hip"))} | {"uvs_pack"}


def test_unit_table_is_the_hip_sources():
    csrc = os.path.join(ROOT, "uv-slam_amd", "csrc")
    on_disk = sorted(f[:-4] for f in os.listdir(csrc) if f.endswith(".hip"))
    table = [row[0] for row in entry.UNITS]
    assert sorted(table) == on_disk
    assert len(set(table)) == len(table)
    # ... and the host-only sources: every *.cpp of csrc/ is linked into the library, and build() names each of them once
    assert sorted(entry.HOST_UNITS) == sorted(f[:-4] for f in os.listdir(csrc) if f.endswith(".cpp"))
    assert len(set(entry.HOST_UNITS)) == len(entry.HOST_UNITS) and not set(entry.HOST_UNITS) & set(table)
    assert sorted(f for f in os.listdir(csrc) if f.endswith((".hip", ".cpp", ".c", ".cc", ".cu"))) == sorted([t + ".hip" for t in table] + [t + ".cpp" for t in entry.HOST_UNITS])


def test_variant_build_names_no_front_end_unit():
    with open(os.path.join(ROOT, "tools", "ab", "build_variant.sh")) as f:
        script = f.read()
    assert REBUILT_BY_VARIANT >= set(entry.HOST_UNITS)      # the packing depends on the -D flags a variant passes (UVS_GLANES): never linked from build()'s object
    front_end = [row[0] for row in entry.UNITS if row[0] not in REBUILT_BY_VARIANT]
    assert len(front_end) >= 7
    named = [stem for stem in front_end if re.search(rf"\b{stem}\b", script)]
    assert named == []
    for stem in REBUILT_BY_VARIANT:      # it does rebuild, and leave out of the link, exactly these
        assert f"{stem}.{'cpp' if stem in entry.HOST_UNITS else 'hip'}" in script and f"{stem}.o" in script
