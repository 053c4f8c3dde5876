"""Host side of the abundance spectrum and the count-range views (no GPU): the five calls are
declared in include/fastkmer.h, exported by the library and bound by the package; a null context is
refused; the ABI version is unchanged; the CLI's new environment variables leave its usage and
configuration errors as they were."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import fastkmer_amd as fk

NEW = ["fk_spectrum", "fk_spectrum_device", "fk_bin_sizes_range", "fk_get_bin_range", "fk_write_bins_range"]


@pytest.fixture(scope="module", autouse=True)
def built():
    from fastkmer_amd import build
    build.build()


def test_the_five_calls_are_declared_exported_and_bound():
    assert set(NEW) <= set(fk.header_functions())
    out = subprocess.check_output(["nm", "-D", "--defined-only", fk.LIB_PATH]).decode()
    exported = {line.split()[-1] for line in out.splitlines() if " T " in line}
    assert set(NEW) <= exported
    L = fk.lib()
    for name in NEW:
        fn = getattr(L, name)
        assert fn.restype is ctypes.c_int and fn.argtypes, name
    # the bound argument counts are the header's
    with open(fk.HEADER_PATH) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    for name in NEW:
        args = re.search(r"\b%s\s*\((.*?)\);" % name, text, re.S).group(1)
        assert len(getattr(L, name).argtypes) == len(args.split(",")), name


def test_abi_version_is_still_3():
    assert fk.lib().fk_abi_version() == 3 == fk.ABI_VERSION
    with open(fk.HEADER_PATH) as f:
        assert "#define FK_ABI_VERSION 3" in f.read()


def test_a_null_context_is_invalid():
    L = fk.lib()
    hist = np.zeros(8, dtype=np.uint64)
    sizes = np.zeros(4096, dtype=np.uint64)
    keys = np.zeros(8, dtype=np.uint64)
    counts = np.zeros(8, dtype=np.uint32)
    n = ctypes.c_size_t(7)
    tail = ctypes.c_uint64(7)
    assert L.fk_spectrum(None, hist.ctypes.data, 8, ctypes.byref(tail)) == -1
    assert L.fk_spectrum_device(None, hist.ctypes.data, 8, None) == -1
    assert L.fk_bin_sizes_range(None, 1, fk.MAX_COUNT, sizes.ctypes.data) == -1
    assert L.fk_get_bin_range(None, 0, 1, fk.MAX_COUNT, keys.ctypes.data, counts.ctypes.data, 8, ctypes.byref(n)) == -1
    assert L.fk_write_bins_range(None, b"/nonexistent/never-made", 1, fk.MAX_COUNT) == -1
    assert L.fk_last_error()
    assert not os.path.exists("/nonexistent")
    assert not hist.any() and tail.value == 7 and n.value == 7  # nothing was written


def test_python_keywords_default_to_the_unfiltered_calls():
    import inspect
    for name in ("bin_sizes", "get_bin", "bin_dict", "bin_text", "write_bins"):
        p = inspect.signature(getattr(fk.KmerCounter, name)).parameters
        assert p["min_count"].default == 1 and p["max_count"].default is None, name
    p = inspect.signature(fk.KmerCounter.spectrum).parameters
    assert p["n"].default == 256 and p["return_tail"].default is False
    assert inspect.signature(fk.KmerCounter.spectrum_ptr).parameters["d_tail"].default == 0
    assert fk._count_range(1, None) is None and fk._count_range(1, fk.MAX_COUNT) is None
    assert fk._count_range(2, None) == (2, fk.MAX_COUNT) and fk._count_range(1, 1) == (1, 1)
    with pytest.raises(ValueError):
        fk._count_range(1, 1 << 32)


def test_cli_errors_are_unchanged_by_the_new_variables():
    env = dict(os.environ, FASTKMER_CLI_MIN_COUNT="2", FASTKMER_CLI_MAX_COUNT="100", FASTKMER_CLI_SPECTRUM="256")
    r = subprocess.run([fk.CLI_PATH], capture_output=True, env=env)
    assert r.returncode == 2 and b"usage" in r.stderr
    bad = [fk.CLI_PATH, "28", "16", "3", "2048", "0", "0", "in", "out", "p", "0", "0", "0"]
    r = subprocess.run(bad, capture_output=True, env=env)
    assert r.returncode == 1 and b"invalid configuration" in r.stderr
    # a malformed value of a new variable is a configuration error too, before any input is read
    ok = [fk.CLI_PATH, "28", "10", "3", "2048", "0", "0", "/nonexistent/in.fa", "out", "p", "0", "0", "0"]
    for name, value in (("FASTKMER_CLI_MIN_COUNT", "0"), ("FASTKMER_CLI_MAX_COUNT", "x"),
                        ("FASTKMER_CLI_SPECTRUM", "1"), ("FASTKMER_CLI_MIN_COUNT", "-3")):
        e = {k: v for k, v in os.environ.items() if not k.startswith("FASTKMER_CLI_")}
        e[name] = value
        r = subprocess.run(ok, capture_output=True, env=e)
        assert r.returncode == 1 and b"invalid configuration" in r.stderr and name.encode() in r.stderr, (name, value)
    e = dict(os.environ, FASTKMER_CLI_MIN_COUNT="5", FASTKMER_CLI_MAX_COUNT="4")
    r = subprocess.run(ok, capture_output=True, env=e)
    assert r.returncode == 1 and b"invalid configuration" in r.stderr


def test_jni_declares_the_two_new_natives():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    scala = open(os.path.join(root, "jni", "skc", "gpu", "NativeKmerCounter.scala")).read()
    c_src = open(os.path.join(root, "jni", "fastkmer_jni.c")).read()
    assert "@native def spectrum(h: Long, n: Int): Array[Long]" in scala
    assert "@native def writeBinsRange(h: Long, outDir: String, minCount: Long, maxCount: Long): Unit" in scala
    for fn, call in (("spectrum", "fk_spectrum("), ("writeBinsRange", "fk_write_bins_range(")):
        assert "Java_skc_gpu_NativeKmerCounter_00024_%s(" % fn in c_src and call in c_src
