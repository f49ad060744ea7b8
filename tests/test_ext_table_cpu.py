"""CPU tier of the extension table (_lib._EXTS), and the only place that pins it: the table is csrc/Makefile's one
`EXTS :=` line (no `EXTS +=` line anywhere) and every name has its NAME_DEPS line there, every row binds exactly what
its header declares and its binary exports, with the types declared — an entry added to a header without a row
of argtypes would otherwise load with ctypes' defaults, int arguments and all —, every loader hands out one library object, and a library of another version or none at all is an ImportError that says what to do.  What is specific
to one library (its literal names and argument types, its refusals) is in that library's own file.  Nothing here touches
a GPU."""
import ctypes
import os
import re

import pytest
from abi_util import declared_functions, exported

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# csrc/Makefile's EXTS, in its order: a new library is a name here, a name there and a row in _lib._EXTS
EXTS = ["augment", "augstep", "auggrid", "depth16", "obb", "lowp", "maplowp", "mapstep", "locate", "accurate", "mapaccurate"]


def test_the_table_has_a_row_and_a_loader_per_extension(pkg):
    assert list(pkg._lib._EXTS) == EXTS
    makefile = open(os.path.join(ROOT, "handposeestimation-with-3d-cnns_amd", "csrc", "Makefile")).read()
    assert re.search(r"^EXTS := (.*)$", makefile, flags=re.M).group(1).split() == EXTS
    for name in EXTS:
        ext = pkg._lib._EXTS[name]
        assert isinstance(ext, pkg._lib._Ext)
        assert ext.path == getattr(pkg._lib, name.upper() + "_LIB_PATH")
        assert ext.version == getattr(pkg._lib, name.upper() + "_VERSION")


def test_one_table_one_exts_line_and_a_deps_line_per_name(pkg):
    assert not hasattr(pkg._lib, "_EXTS2")                                                 # one table
    lines = open(os.path.join(ROOT, "handposeestimation-with-3d-cnns_amd", "csrc", "Makefile")).read().splitlines()
    at = [k for k, ln in enumerate(lines) if re.match(r"^EXTS := ", ln)]
    assert len(at) == 1 and lines[at[0]].split(":=")[1].split() == EXTS
    assert not [ln for ln in lines if re.match(r"^\s*EXTS\s*\+=", ln)]                      # and one line that fills it
    assert min(k for k, ln in enumerate(lines) if "$(EXTS)" in ln and not ln.startswith("#")) > at[0]
    for name in EXTS:
        assert any(re.match(rf"^{name}_DEPS := ", ln) for ln in lines), name


@pytest.mark.parametrize("name", EXTS)
def test_row_binds_exactly_its_header_with_types(pkg, name):
    ext = pkg._lib._EXTS[name]
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


@pytest.mark.parametrize("name", EXTS)
def test_loading_twice_gives_the_same_object(pkg, name):
    load = getattr(pkg._lib, "load_" + name)
    assert load() is load()
    assert load() is not pkg._lib.load()
    assert all(load() is not getattr(pkg._lib, "load_" + other)() for other in EXTS if other != name)


@pytest.mark.parametrize("name", EXTS)
def test_wrong_version_and_missing_library_raise_import_error(pkg, monkeypatch, name):
    row = pkg._lib._EXTS[name]
    load = getattr(pkg._lib, "load_" + name)
    monkeypatch.delitem(pkg._lib._ext_libs, name, raising=False)
    monkeypatch.setitem(pkg._lib._EXTS, name, row._replace(version=row.version + 1))
    with pytest.raises(ImportError, match="version 1"):
        load()
    monkeypatch.setitem(pkg._lib._EXTS, name, row._replace(path=os.path.join(ROOT, "build", f"no_such_libtsdf_{name}.so")))
    with pytest.raises(ImportError, match=f"csrc {name}"):
        load()
