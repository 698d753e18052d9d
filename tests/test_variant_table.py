"""tools/variant_sweep.py's tuning table names only switches the sources still have (CPU, no build).

A define `RT_NAME[=v]` in VARIANTS, or a FIELDS macro, must be a macro that some file under csrc/ reads:
a build with a name nothing reads is the default build under another label, and an A/B of it measures
noise. Compiler flags (`-...`, `@<source>:<flag>`) are not defines; `@<source>` must be one of
build.SOURCES (build._extra_flags drops a flag for a source it does not compile)."""
import importlib.util
import re
from pathlib import Path

import pytest

from distraytracer_old_amd import build

REPO = Path(__file__).resolve().parents[1]


def _sweep():
    spec = importlib.util.spec_from_file_location("variant_sweep", REPO / "tools" / "variant_sweep.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


SWEEP = _sweep()
# every RT_* identifier the sources mention outside comments
_SRC = "\n".join(re.sub(r"//[^\n]*|/\*.*?\*/", "", p.read_text(), flags=re.S) for p in sorted(build.CSRC.iterdir())
                 if p.suffix in (".h", ".hip", ".cpp", ".c"))
READ = set(re.findall(r"\bRT_[A-Z0-9_]+\b", _SRC))


def _macros(defines):
    for d in defines:
        if d.startswith("@"):
            src, flag = d[1:].split(":", 1)
            assert src in build.SOURCES, f"{d}: {src} is not a source of the build"
            assert flag.startswith("-") and not flag.startswith("-D"), f"{d}: per-source flags are compiler flags"
        elif d.startswith("-D") or not d.startswith("-"):  # a define, bare or spelled as the compiler's -D
            m = re.fullmatch(r"(?:-D)?(RT_[A-Z0-9_]+)(=.*)?", d)
            assert m, f"{d!r} is neither a compiler flag nor an RT_* define"
            yield m.group(1)


def test_dash_d_counts_as_a_define():
    assert list(_macros(["-DRT_STACK_LDS=8", "RT_PK_LDS", "-O2", "@trace.hip:-O1"])) == ["RT_STACK_LDS", "RT_PK_LDS"]


def test_the_sources_are_read():
    assert {"RT_STACK_LDS", "RT_PROF_REGIONS", "RT_RENDER_WAVES"} <= READ  # the scan itself finds the kept switches


@pytest.mark.parametrize("name", sorted(SWEEP.VARIANTS))
def test_variant_defines_are_read(name):
    missing = [m for m in _macros(SWEEP.VARIANTS[name]) if m not in READ]
    assert not missing, f"variant {name!r} sets {missing}: no file under csrc/ reads it"


def test_field_macros_are_read():
    missing = {k: m for k, m in SWEEP.FIELDS.items() if m not in READ}
    assert not missing, f"FIELDS letters {missing}: no file under csrc/ reads these macros"
    for k in SWEEP.FIELDS:  # a parsed name such as "s12w4" resolves through defines_of
        assert SWEEP.defines_of(f"{k}3") == [f"{SWEEP.FIELDS[k]}=3"]


def test_one_default_build():
    empty = [n for n, d in SWEEP.VARIANTS.items() if not d]
    assert empty == ["base"], f"aliases of the default build: {empty}"
