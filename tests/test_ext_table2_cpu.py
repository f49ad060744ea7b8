"""CPU tier of the second extension table (_lib._EXTS2), and the only place that pins it: the libraries added after the nine
of tests/test_ext_table_cpu.py.  The table is csrc/Makefile's `EXTS += name` lines, in their order and directly under the
`EXTS :=` line (before EXT_RES / EXT_ASM are expanded, so the rule template covers them); every row binds exactly what its
header declares and its binary exports, with the types declared; every loader hands out one library object; and a library
of another version or none at all is an ImportError that says what to do.  What is specific to one library is in that
library's own file.  Nothing here touches a GPU."""
import ctypes
import os
import re

import pytest
from abi_util import declared_functions, exported

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# csrc/Makefile's EXTS += lines, in their order: a new library is a name here, a line there and a row in _lib._EXTS2
EXTS2 = ["accurate"]


def test_the_table_has_a_row_and_a_loader_per_extension(pkg):
    assert list(pkg._lib._EXTS2) == EXTS2
    assert not set(pkg._lib._EXTS2) & set(pkg._lib._EXTS)
    lines = open(os.path.join(ROOT, "handposeestimation-with-3d-cnns_amd", "csrc", "Makefile")).read().splitlines()
    at = [k for k, ln in enumerate(lines) if re.match(r"^EXTS := ", ln)]
    assert len(at) == 1
    added = [ln for ln in lines if re.match(r"^EXTS \+= ", ln)]
    assert [ln.split("+=")[1].split() for ln in added] == [[name] for name in EXTS2]      # one name per line
    assert lines[at[0] + 1:at[0] + 1 + len(EXTS2)] == added                                # directly under the := line
    first_use = min(k for k, ln in enumerate(lines) if "$(EXTS)" in ln and not ln.startswith("#"))
    assert first_use > at[0] + len(EXTS2)
    for name in EXTS2:
        ext = pkg._lib._EXTS2[name]
        assert isinstance(ext, pkg._lib._Ext)
        assert ext.path == getattr(pkg._lib, name.upper() + "_LIB_PATH")
        assert ext.version == getattr(pkg._lib, name.upper() + "_VERSION")
        assert any(re.match(rf"^{name}_DEPS := ", ln) for ln in lines), name


@pytest.mark.parametrize("name", EXTS2)
def test_row_binds_exactly_its_header_with_types(pkg, name):
    ext = pkg._lib._EXTS2[name]
    want = sorted([ext.version_symbol, *ext.entries])
    assert want == declared_functions(f"tsdf_{name}.h")
    funcs, named = exported(ext.path)
    assert funcs == want and named == want
    L = getattr(pkg._lib, "load_" + name)()
    assert getattr(L, ext.version_symbol)() == ext.version
    for entry in (ext.version_symbol, *ext.entries):
        fn = getattr(L, entry)
        assert fn.restype is ctypes.c_int, entry
        assert fn.argtypes is not None, entry
    for entry, argtypes in ext.entries.items():
        assert list(getattr(L, entry).argtypes) == argtypes and argtypes, entry


@pytest.mark.parametrize("name", EXTS2)
def test_loading_twice_gives_the_same_object(pkg, name):
    load = getattr(pkg._lib, "load_" + name)
    assert load() is load()
    assert load() is not pkg._lib.load()
    others = [n for n in (*pkg._lib._EXTS, *pkg._lib._EXTS2) if n != name]
    assert all(load() is not getattr(pkg._lib, "load_" + other)() for other in others)


@pytest.mark.parametrize("name", EXTS2)
def test_wrong_version_and_missing_library_raise_import_error(pkg, monkeypatch, name):
    row = pkg._lib._EXTS2[name]
    load = getattr(pkg._lib, "load_" + name)
    monkeypatch.delitem(pkg._lib._ext_libs, name, raising=False)
    monkeypatch.setitem(pkg._lib._EXTS2, name, row._replace(version=row.version + 1))
    with pytest.raises(ImportError, match="version 1"):
        load()
    monkeypatch.setitem(pkg._lib._EXTS2, name, row._replace(path=os.path.join(ROOT, "build", f"no_such_libtsdf_{name}.so")))
    with pytest.raises(ImportError, match=f"csrc {name}"):
        load()
