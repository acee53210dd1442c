"""The parallel JPEG entropy decode restated on the host (tests/jpeg_entropy_host.cpp: the product's prescan and subsequence
step of hpmvs_amd/csrc/jpeg.hpp, with the kernels' rounds, check, sums and write as loops) against decode_file, which
tests/test_cpu_jpeg.py pins to libjpeg: every coefficient of the 20 fixture files at every subsequence size, the rounds that
set the shipped cap, seeded mutations, and the same under AddressSanitizer and UBSan in a stand-alone program."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest

from jpeg_entropy_ref import ROOT, SHIPPED_BITS, SRC, SWEEP, EntropyHost, files, mutation_set


@pytest.fixture(scope="module")
def host(tmp_path_factory):
    return EntropyHost(tmp_path_factory.mktemp("jpeg_entropy_host"))


def _constant(name):
    text = open(os.path.join(ROOT, "hpmvs_amd", "csrc", "jpeg.hpp")).read()
    return int(re.search(r"constexpr int %s = (\d+);" % name, text).group(1))


def test_fixture_is_the_twenty_files():
    names = [n for n, _ in files()]
    assert len(names) == 20 and len(set(names)) == 20
    assert os.path.getsize(os.path.join(ROOT, "tests", "golden", "g8_jpeg_entropy.npz")) < os.path.getsize(
        os.path.join(ROOT, "tests", "golden", "g7_jpeg.npz"))
    assert _constant("kSubseqBits") == SHIPPED_BITS


def test_every_coefficient_at_every_subsequence_size_and_the_round_cap(host):
    """no file falls back; the shipped cap is four times the rounds the slowest file needs at the shipped size"""
    slowest = 0
    for name, data in files():
        rc, truth, msg = host.host(data)
        assert rc == 0, (name, msg)
        rounds = []
        for bits in SWEEP:
            rc, coef, _, accepted, r = host.scheme(data, bits)
            assert rc == 0 and accepted, f"{name}: fell back at {bits} bits after {r} rounds"
            assert np.array_equal(coef, truth), f"{name} at {bits} bits: {int((coef != truth).sum())} coefficients differ"
            rounds.append(r)
        slowest = max(slowest, rounds[-1])
        print(f"\n{name}: rounds at {SWEEP} bits: {rounds}", end="")
    print(f"\nslowest file at {SHIPPED_BITS} bits: {slowest} rounds")
    assert _constant("kSyncRoundCap") == 4 * slowest


def test_a_cap_below_the_rounds_needed_falls_back_to_the_host_coefficients(host):
    big = dict(files())["noise64_444_q100_opt"]
    truth = host.host(big)[1]
    rc, coef, _, accepted, r = host.scheme(big, 0, round_cap=5)
    assert rc == 0 and not accepted and r == 5 and np.array_equal(coef, truth)


def test_mutations_never_differ_from_the_host_and_seldom_fall_back(host):
    """whatever the scheme accepts is the host's; of the mutations the host accepts it may leave 25 % to the host at most"""
    accepted_by_host = fell_back = 0
    for name, k, m in mutation_set():
        rc, truth, msg = host.host(m)
        rc2, coef, msg2, accepted, _ = host.scheme(m)
        assert (rc2, msg2) == (rc, msg), (name, k)
        if rc == 0:
            assert np.array_equal(coef, truth), (name, k)
            accepted_by_host += 1
            fell_back += not accepted
        else:
            assert not accepted, (name, k)
    print(f"\n{accepted_by_host} mutations the host accepts, {fell_back} left to the host")
    assert accepted_by_host >= 400
    assert fell_back <= 0.25 * accepted_by_host


def test_restatement_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """a stand-alone program (its own main): the scheme over the files at every size and over the mutations at two"""
    exe = str(tmp_path / "jpeg_entropy_san")
    subprocess.run(["g++", "-std=c++14", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-DJE_MAIN", SRC,
                    "-o", exe], check=True, capture_output=True)
    for label, records, sizes in (("files", [b for _, b in files()], SWEEP), ("mutations", [m for _, _, m in mutation_set()], [64, SHIPPED_BITS])):
        path = str(tmp_path / (label + ".bin"))
        with open(path, "wb") as f:
            for b in records:
                f.write(struct.pack("<I", len(b)) + b)
        r = subprocess.run([exe, path] + [str(s) for s in sizes], capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, f"{label}: exit {r.returncode}\n{r.stderr[-3000:]}"
        n, host_ok, parallel, fallbacks, mismatches = [int(x) for x in r.stdout.split()]
        print(f"\n{label}: {n} records, {host_ok} accepted by the host, {parallel} parallel decodes, {fallbacks} fallbacks, no sanitizer report")
        assert n == len(records) and mismatches == 0 and parallel > 0
        assert "runtime error" not in r.stderr and "AddressSanitizer" not in r.stderr
