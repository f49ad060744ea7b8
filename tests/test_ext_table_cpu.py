"""CPU tier of the extension table (_lib._EXTS): every row binds exactly what its header declares, with the types
declared — an entry added to a header without a row of argtypes would otherwise load with ctypes' defaults, int arguments
and all —, every loader hands out one library object, and a library of another version or none at all is an ImportError
that says what to do.  Nothing here touches a GPU."""
import ctypes
import os

import pytest
from abi_util import declared_functions

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXTS = ["augment", "augstep", "auggrid", "depth16", "obb", "lowp"]   # csrc/Makefile's EXTS, in its order


def test_the_table_has_a_row_and_a_loader_per_extension(pkg):
    assert list(pkg._lib._EXTS) == EXTS
    for name in EXTS:
        ext = pkg._lib._EXTS[name]
        assert ext.path == getattr(pkg._lib, name.upper() + "_LIB_PATH")
        assert ext.version == getattr(pkg._lib, name.upper() + "_VERSION")


@pytest.mark.parametrize("name", EXTS)
def test_row_binds_exactly_its_header_with_types(pkg, name):
    ext = pkg._lib._EXTS[name]
    assert sorted([ext.version_symbol, *ext.entries]) == declared_functions(f"tsdf_{name}.h")
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
