"""CPU tier of the extension table (_lib._EXTS): every row binds exactly what its header declares, with the types
declared — an entry added to a header without a row of argtypes would otherwise load with ctypes' defaults, int arguments
and all — and every loader hands out one library object.  Nothing here touches a GPU."""
import ctypes

import pytest
from abi_util import declared_functions

EXTS = ["augment", "augstep", "auggrid", "depth16"]


def test_the_table_has_a_row_and_a_loader_per_extension(pkg):
    assert sorted(pkg._lib._EXTS) == sorted(EXTS)
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
