"""The host stack over a stand-in library, for tests that check control flow WITHOUT a GPU: the stand-in is built from the
fake_msegk*.c files of this directory, medicalseg_amd is imported afresh with _lib.LIB_PATH pointing at it, and everything is
put back afterwards.  The first import of the package still loads the library _lib.LIB_PATH names at that moment, so a built
libmsegk.so (./build.sh) or MSEGK_LIB=<any library that loads> is needed, as it was for the fixtures this module replaces.  A
test module takes what it needs:

    fake_pkg = fake_lib.fake_pkg_fixture("fake_msegk.c", "fake_msegk_region.c")
    from fake_lib import calls, fake
"""
import contextlib
import os
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def _purge():
    for m in [k for k in sys.modules if k.startswith("medicalseg_amd")]:
        del sys.modules[m]


@contextlib.contextmanager
def standin(directory, *sources):
    """medicalseg_amd over the stand-in built from `sources` into `directory`; yields the package"""
    so = os.path.join(str(directory), "libfake_msegk.so")
    subprocess.check_call(["gcc", "-shared", "-fPIC", "-O1", "-w", "-o", so] + [os.path.join(HERE, s) for s in sources])
    _purge()
    import importlib
    lib = importlib.import_module("medicalseg_amd._lib")
    real = lib.LIB_PATH
    lib.LIB_PATH = so
    lib._lib = None
    import medicalseg_amd
    from medicalseg_amd.device import Device
    Device._current = None
    try:
        yield medicalseg_amd
    finally:
        lib.LIB_PATH = real
        lib._lib = None
        Device._current = None
        _purge()


def fake_pkg_fixture(*sources):
    """a module-scoped fixture that holds standin(*sources) open"""
    @pytest.fixture(scope="module")
    def fake_pkg(tmp_path_factory):
        with standin(tmp_path_factory.mktemp("fake"), *sources) as pkg:
            yield pkg
    return fake_pkg


@pytest.fixture
def calls(fake_pkg, monkeypatch):
    """names of the library calls made through Device.call, in order"""
    from medicalseg_amd.device import Device
    names = []
    real = Device.call

    def recording(self, name, *args):
        names.append(name)
        return real(self, name, *args)
    monkeypatch.setattr(Device, "call", recording)
    return names


def fake(name, restype, *args):
    """call one of the stand-in's own inspection functions"""
    from medicalseg_amd import _lib
    fn = getattr(_lib.load(), name)
    fn.restype = restype
    return fn(*args)
