"""Host side of the two-sample comparison (no GPU): the four calls are declared in include/fastkmer.h,
exported by the library and bound by the package; a null context on either side is refused; the ABI
version is unchanged; the CLI's new environment variables fail as usage errors before any device is
touched and leave its other usage and configuration errors as they were."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import fastkmer_amd as fk

NEW = ["fk_compare", "fk_compare_device", "fk_bin_sizes_joined", "fk_get_bin_joined"]
MAX = fk.MAX_COUNT


@pytest.fixture(scope="module", autouse=True)
def built():
    from fastkmer_amd import build
    build.build()


def test_the_four_calls_are_declared_exported_and_bound():
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
    assert "two-sample comparison (no reference counterpart)" in open(fk.HEADER_PATH).read()


def test_abi_version_is_still_3():
    assert fk.lib().fk_abi_version() == 3 == fk.ABI_VERSION
    with open(fk.HEADER_PATH) as f:
        assert "#define FK_ABI_VERSION 3" in f.read()


def test_a_null_context_on_either_side_is_invalid():
    L = fk.lib()
    mat = np.zeros(16, dtype=np.uint64)
    sizes = np.zeros(4096, dtype=np.uint64)
    keys = np.zeros(8, dtype=np.uint64)
    counts = np.zeros(8, dtype=np.uint32)
    others = np.zeros(8, dtype=np.uint32)
    n = ctypes.c_size_t(7)
    fake = ctypes.c_void_p(mat.ctypes.data)  # never dereferenced: the null side is refused first
    for ctx, other in ((None, None), (None, fake), (fake, None)):
        assert L.fk_compare(ctx, other, mat.ctypes.data, 4, 4) == -1
        assert L.fk_compare_device(ctx, other, mat.ctypes.data, 4, 4) == -1
        assert L.fk_bin_sizes_joined(ctx, other, 1, MAX, 0, MAX, sizes.ctypes.data) == -1
        assert L.fk_get_bin_joined(ctx, other, 0, 1, MAX, 0, MAX, keys.ctypes.data, counts.ctypes.data,
                                   others.ctypes.data, 8, ctypes.byref(n)) == -1
        assert L.fk_last_error()
    assert not mat.any() and not sizes.any() and not keys.any() and n.value == 7  # nothing was written


def test_python_methods_and_their_defaults():
    p = inspect.signature(fk.KmerCounter.compare).parameters
    assert p["rows"].default == 256 and p["cols"].default == 256
    assert list(inspect.signature(fk.KmerCounter.compare_ptr).parameters) == ["self", "other", "d_matrix", "rows", "cols"]
    for name in ("bin_sizes_joined", "get_bin_joined"):
        p = inspect.signature(getattr(fk.KmerCounter, name)).parameters
        assert (p["min_count"].default, p["max_count"].default, p["other_min"].default, p["other_max"].default) == \
            (1, None, 0, None), name
    for name in ("intersect_bin", "subtract_bin"):
        assert list(inspect.signature(getattr(fk.KmerCounter, name)).parameters) == ["self", "other", "b"]
    assert fk.KmerCounter._join_range(1, None, 0, None) == (1, MAX, 0, MAX)
    assert fk.KmerCounter._join_range(2, 3, 1, 1) == (2, 3, 1, 1)
    with pytest.raises(ValueError):
        fk.KmerCounter._join_range(1, None, 0, 1 << 32)


ARGS = ["28", "10", "3", "2048", "0", "0", "/nonexistent/in.fa", "out", "p", "0", "0", "0"]


def _clean_env(**extra):
    e = {k: v for k, v in os.environ.items() if not k.startswith("FASTKMER_CLI_")}
    e.update(extra)
    return e


def test_cli_compare_usage_errors_come_before_any_device():
    # no device is made visible: a run that got as far as fk_create would fail differently
    hidden = dict(HIP_VISIBLE_DEVICES="", ROCR_VISIBLE_DEVICES="")
    with_ht = ARGS[:4] + ["1"] + ARGS[5:]
    r = subprocess.run([fk.CLI_PATH] + with_ht, capture_output=True,
                       env=_clean_env(FASTKMER_CLI_COMPARE="/nonexistent/other.fa", **hidden))
    assert r.returncode == 2 and b"usage" in r.stderr and b"FASTKMER_CLI_COMPARE" in r.stderr and b"useHT = 0" in r.stderr
    for n in ("1", "4097", "x", "-3"):
        for extra in ({}, {"FASTKMER_CLI_COMPARE": "/nonexistent/other.fa"}):
            r = subprocess.run([fk.CLI_PATH] + ARGS, capture_output=True,
                               env=_clean_env(FASTKMER_CLI_COMPARE_N=n, **hidden, **extra))
            assert r.returncode == 2 and b"usage" in r.stderr and b"FASTKMER_CLI_COMPARE_N" in r.stderr, (n, extra)
    # a well-formed pair gets past the checks: the missing input is what fails
    r = subprocess.run([fk.CLI_PATH] + ARGS, capture_output=True,
                       env=_clean_env(FASTKMER_CLI_COMPARE="/nonexistent/other.fa", FASTKMER_CLI_COMPARE_N="2", **hidden))
    assert r.returncode == 1 and b"cannot open /nonexistent/in.fa" in r.stderr


def test_cli_errors_without_the_new_variables_are_unchanged():
    env = _clean_env()
    r = subprocess.run([fk.CLI_PATH], capture_output=True, env=env)
    assert r.returncode == 2 and b"usage" in r.stderr
    bad = [fk.CLI_PATH, "28", "16", "3", "2048", "0", "0", "in", "out", "p", "0", "0", "0"]
    r = subprocess.run(bad, capture_output=True, env=env)
    assert r.returncode == 1 and b"invalid configuration" in r.stderr
    r = subprocess.run([fk.CLI_PATH] + ARGS, capture_output=True, env=env)
    assert r.returncode == 1 and b"cannot open /nonexistent/in.fa" in r.stderr and b"usage" not in r.stderr
    # ... and the older variables' errors stay what they were beside a comparison request
    for name, value in (("FASTKMER_CLI_MIN_COUNT", "0"), ("FASTKMER_CLI_SPECTRUM", "1")):
        r = subprocess.run([fk.CLI_PATH] + ARGS, capture_output=True,
                           env=_clean_env(FASTKMER_CLI_COMPARE="/nonexistent/other.fa", **{name: value}))
        assert r.returncode == 1 and b"invalid configuration" in r.stderr and name.encode() in r.stderr, name
    with_ht = ARGS[:4] + ["1"] + ARGS[5:]
    r = subprocess.run([fk.CLI_PATH] + with_ht, capture_output=True, env=_clean_env(FASTKMER_CLI_READS="/nonexistent/r.fa"))
    assert r.returncode == 2 and b"FASTKMER_CLI_READS needs the sorted count" in r.stderr
