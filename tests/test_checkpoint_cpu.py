"""Checkpoint and restart on the CPU: the blob's writer, reader and validator and the host digest (csrc/hdg_checkpoint.hpp through
tests/host/checkpoint_check.cpp, g++ with AddressSanitizer and UBSan), the numpy restatement of the digest, the C-ABI table of
include/hdg_checkpoint.h and the driver's options.  No GPU and no built library are needed."""
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import checkpoint_reference as ref

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def test_blob_round_trip_truncations_bounds_and_host_digest(tmp_path):
    """The stand-alone program over csrc/hdg_checkpoint.hpp, built with -fsanitize=address,undefined: a synthetic blob comes back
    field by field; each of its shorter prefixes is refused (every buffer is an exact-size heap copy: a read past the end would
    stop the program); table entries that leave the file, wrap around or point into the header are refused by section name;
    bad magic, another version and one flipped byte per section are named; the host digest of fixed words equals the numpy
    restatement as integers."""
    gxx = shutil.which("g++")
    if gxx is None:
        pytest.skip("no g++")
    exe = tmp_path / "checkpoint_check"
    subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-o", str(exe), os.path.join(HERE, "host", "checkpoint_check.cpp")], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr
    got = {int(m[0]): (int(m[1]), int(m[2])) for m in re.findall(r"^digest (\d+) (\d+) (\d+)$", r.stdout, re.M)}
    assert sorted(got) == [0, 1, 2, 5, 64, 1000]
    for n, d in got.items():
        assert d == ref.digest(ref.fixed_words(n)), n
    m = re.search(r"^digest_bytes 11 (\d+) (\d+)$", r.stdout, re.M)
    assert (int(m[1]), int(m[2])) == ref.digest_bytes(bytes(range(1, 12)))
    m = re.search(r"truncations refused (\d+) of (\d+)", r.stdout)
    assert m[1] == m[2] and int(m[2]) > 500


def test_reference_digest_is_the_formula():
    """The numpy restatement against the definition in Python integers, the wrap included, and the two properties the odd
    weights give: one changed word and a swap of two unequal words change the digest."""
    for kind in ref.KINDS:
        v = ref.patterns(kind, 257)
        b = [int(x) for x in v.view(np.uint64)]
        d0 = sum(b) % 2 ** 64
        d1 = sum(x * (2 * i + 1) for i, x in enumerate(b)) % 2 ** 64
        assert ref.digest(v) == (d0, d1), kind
    assert ref.digest(np.zeros(0)) == (0, 0)
    assert ref.digest(ref.patterns("ones", 4)) == ((2 ** 64 - 4) % 2 ** 64, (-16) % 2 ** 64)
    v = ref.patterns("random", 100).copy()
    d = ref.digest(v)
    w = v.copy()
    w[[3, 77]] = w[[77, 3]]
    assert ref.digest(w)[0] == d[0] and ref.digest(w)[1] != d[1]
    w = v.view(np.uint64).copy()
    w[10] ^= np.uint64(1 << 40)
    assert ref.digest(w)[0] != d[0]
    assert len(ref.LENGTHS) == 12 and ref.LENGTHS[-1] > ref.GRID_WORDS


SIGNATURES_IN_C = {
    "hdg_checkpoint_size": "int hdg_checkpoint_size(hdg_handle* h, long* nbytes);",
    "hdg_checkpoint_save": "int hdg_checkpoint_save(hdg_handle* h, long step, double t, void* buf, long nbytes);",
    "hdg_checkpoint_load": "int hdg_checkpoint_load(hdg_handle* h, const void* buf, long nbytes, long* step, double* t);",
    "hdg_state_digest": "int hdg_state_digest(hdg_handle* h, unsigned long long out[2]);",
    "hdg_digest_vector": "int hdg_digest_vector(hdg_handle* h, const double* v, long n, unsigned long long out[2]);",
}


def test_c_abi_declares_the_checkpoint_entry_points_in_their_own_header():
    import ctypes as C

    from incompressibleeulerhdg_amd import _lib

    assert set(_lib.CHECKPOINT_SIGNATURES) == set(SIGNATURES_IN_C)
    header = open(os.path.join(ROOT, "include", "hdg_checkpoint.h")).read()
    main_header = open(os.path.join(ROOT, "include", "hdg_mi355x.h")).read()
    for name, decl in SIGNATURES_IN_C.items():
        assert decl in header, name
        assert name not in main_header and name not in _lib.SIGNATURES, name
    # the functions the new header declares are exactly the table
    assert set(re.findall(r"^int (hdg_\w+)\(", header, re.M)) == set(SIGNATURES_IN_C)
    # argument types of the binding, one by one
    h, lp, dp, ullp = C.c_void_p, C.POINTER(C.c_long), C.POINTER(C.c_double), C.POINTER(C.c_ulonglong)
    assert _lib.CHECKPOINT_SIGNATURES["hdg_checkpoint_size"] == [h, lp]
    assert _lib.CHECKPOINT_SIGNATURES["hdg_checkpoint_save"] == [h, C.c_long, C.c_double, C.c_void_p, C.c_long]
    assert _lib.CHECKPOINT_SIGNATURES["hdg_checkpoint_load"] == [h, C.c_void_p, C.c_long, lp, dp]
    assert _lib.CHECKPOINT_SIGNATURES["hdg_state_digest"] == [h, ullp]
    assert _lib.CHECKPOINT_SIGNATURES["hdg_digest_vector"] == [h, dp, C.c_long, ullp]
    # the engine defines them, and the binding's view of the blob header is the C++ struct's
    engine = open(os.path.join(ROOT, "incompressibleeulerhdg_amd", "csrc", "hdg_engine.hip")).read()
    for name in SIGNATURES_IN_C:
        assert re.search(rf"^int {name}\(", engine, re.M), name
    import struct

    assert struct.calcsize(_lib.Engine._CK_HEADER) == 64
    with pytest.raises(ValueError, match="not a checkpoint"):
        _lib.Engine.checkpoint_info(b"short")
    blob = struct.pack(_lib.Engine._CK_HEADER, b"HDGCKPT\0", 1, 0, 7, 0.5, 64, 0, 8, 64, 1 | 4 | 8)
    info = _lib.Engine.checkpoint_info(blob)
    assert info == dict(tracer=True, diagnostics=False, probes=True, particles=True, step=7, t=0.5, n_probes=8, n_particles=64)


def test_solve_takes_the_checkpoint_keywords_last_and_off():
    import inspect

    from incompressibleeulerhdg_amd import timesteppers as ts

    for cls in (ts.IncompressibleEulerHDGIMEXSSP2_332, ts.IncompressibleEulerHDGImplicit, ts.IncompressibleEulerDGImplicit):
        p = inspect.signature(cls.solve).parameters
        assert list(p)[-3:] == ["checkpoint", "checkpoint_every", "restart"], cls
        assert p["checkpoint"].default is None and not p["checkpoint_every"].default and p["restart"].default is None


def test_driver_parses_checkpoint_options_and_refuses_before_any_engine(tmp_path, monkeypatch):
    from incompressibleeulerhdg_amd import driver

    args = driver.build_parser().parse_args([])
    assert args.checkpoint is None and args.checkpoint_every is None and args.restart is None
    driver.check_checkpoint(args)
    args = driver.build_parser().parse_args(["--checkpoint", "c.bin", "--checkpoint_every", "5", "--restart", "r.bin"])
    assert (args.checkpoint, args.checkpoint_every, args.restart) == ("c.bin", 5, "r.bin")

    # nothing below may start a rank or build an engine
    def boom(*a, **k):
        raise AssertionError("a refusal came too late")

    monkeypatch.setattr(driver, "launch_ranks", boom)
    monkeypatch.setattr(driver, "_Ranks", boom)
    monkeypatch.setattr(driver, "_run", boom)
    for m in ("0", "-3"):
        with pytest.raises(RuntimeError, match="--checkpoint_every must be at least 1"):
            driver.main(["--checkpoint", str(tmp_path / "c.bin"), "--checkpoint_every", m])
    there = tmp_path / "there.bin"
    there.write_bytes(b"x")
    with pytest.raises(RuntimeError, match="--restart does not go with --warmup"):
        driver.main(["--restart", str(there), "--warmup"])
    with pytest.raises(RuntimeError, match="--restart does not go with --test_pressure_solver"):
        driver.main(["--restart", str(there), "--test_pressure_solver"])
    with pytest.raises(RuntimeError, match="no checkpoint file .*missing.bin"):
        driver.main(["--restart", str(tmp_path / "missing.bin")])
    # strips: every rank's file is looked for before a rank is started
    (tmp_path / "s.bin.0").write_bytes(b"x")
    with pytest.raises(RuntimeError, match=r"no checkpoint file .*s\.bin\.1"):
        driver.main(["--problem", "shear", "--nx", "16", "--gpus", "2", "--restart", str(tmp_path / "s.bin")])
    with pytest.raises(AssertionError, match="too late"):  # a request that is fine does go on
        driver.main(["--restart", str(there)])
