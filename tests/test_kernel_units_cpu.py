"""tools/compare_kernel_asm.py takes its translation units from csrc/Makefile: the list is complete and follows the Makefile.  No GPU, no build."""
import importlib.util
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "fsw_gnn_amd", "csrc")

_spec = importlib.util.spec_from_file_location("compare_kernel_asm", os.path.join(ROOT, "tools", "compare_kernel_asm.py"))
tool = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(tool)

MAKEFILE_TEXT = open(os.path.join(CSRC, "Makefile")).read()


def test_units_cover_every_source_file():
    units = tool.units_of(MAKEFILE_TEXT)
    assert units and units == tool.UNITS
    names = [name for _, _, name in units]
    assert len(names) == len(set(names)), "unit names are output file names"
    sources = {src for src, _, _ in units}
    for src in sources:
        assert os.path.isfile(os.path.join(CSRC, src + ".hip")), src
    on_disk = {f[:-4] for f in os.listdir(CSRC) if f.endswith(".hip")}
    assert on_disk <= sources, "in no unit: %s" % sorted(on_disk - sources)


def test_part_units_carry_their_define():
    units = tool.units_of(MAKEFILE_TEXT)
    parts = [u for u in units if u[2] != u[0]]
    assert parts, "embed_mid, embed_mid_bwd and embed_hub are built in parts"
    for src, define, name in parts:
        number = name[len(src) + 1:]
        assert name == "%s_%s" % (src, number) and number.isdigit()
        assert re.fullmatch(r"-D\w+=%s" % number, define), (name, define)
    for src, define, name in units:
        if name == src:
            assert define == ""
    # every part object of OBJS is a unit
    part_objects = set(re.findall(r"\$\(OBJDIR\)/(\w+_\d+)\.o", MAKEFILE_TEXT))
    assert part_objects == {name for _, _, name in parts}


def test_a_new_source_file_appears_by_srcs_alone():
    before = tool.units_of(MAKEFILE_TEXT)
    changed = re.sub(r"^(SRCS\s*:=.*)$", r"\1 brand_new_kernel.hip", MAKEFILE_TEXT, count=1, flags=re.M)
    assert changed != MAKEFILE_TEXT
    after = tool.units_of(changed)
    assert ("brand_new_kernel", "", "brand_new_kernel") in after
    assert [u for u in after if u[0] != "brand_new_kernel"] == before
