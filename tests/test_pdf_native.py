"""CPU: rt_pdf.h as a program of its own (tests/native/pdf_levels.cpp, plain and under the sanitizers) agrees with
tests/pdf_ref.py bit for bit: the host finalisation of an event's integer sums -- moments, ellipse, area, rim fraction and the
walk of the histogram for every level, including an empty histogram, a level reached in the top bin and sums past 2^64 -- and
the density, the mass, the bin and the sample quantum of single values.  DESIGN.md section 33."""
import os
import subprocess

import numpy as np
import pytest

import pdf_ref
from conftest import ROOT
from test_pdf_host import GRID, LEVELS, gaussian_obj, l2_case


@pytest.fixture(scope="module")
def programs(tmp_path_factory):
    d = tmp_path_factory.mktemp("pdf_levels")
    src = os.path.join(ROOT, "tests", "native", "pdf_levels.cpp")
    out = {}
    for name, flags in (("plain", []), ("san", ["-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g"])):
        exe = str(d / name)
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-ffp-contract=off", "-Wall"] + flags + ["-o", exe, src])
        out[name] = exe
    return out


def hx(v):
    return float(v).hex()


def unhx(s):
    return float("nan") if "nan" in s else float.fromhex(s)


def final_cases():
    """(name, sums, count, mass, ix, iy, levels)"""
    cases = []
    maps = {"gaussian": gaussian_obj(18.3, 13.6, 2.5, 1.8),
            "two_lobes": np.minimum(gaussian_obj(9.0, 8.0, 2.0, 1.5), 0.3 + gaussian_obj(27.2, 20.1, 1.5, 2.5)),
            "on_the_rim": gaussian_obj(0.0, 14.0, 2.0, 1.5), "top_bin": gaussian_obj(36.0, 28.0, 0.1, 0.1)}
    i, j = np.arange(37)[None, :], np.arange(29)[:, None]
    maps["tilted"] = ((i - 18.0) + (j - 14.0)) ** 2 / 9.0 + ((i - 18.0) - (j - 14.0)) ** 2 / 2.0
    for name, obj in maps.items():
        o, node = l2_case(obj)
        count, mass = o["hist"][0]
        cases.append((name, o["sums"][0], count, mass, node % 37, node // 37, LEVELS))
    s, count, mass = cases[0][1:4]
    cases.append(("no_levels", s, count, mass, 18, 14, ()))
    cases.append(("eight_levels", s, count, mass, 18, 14, (0.01, 0.1, 0.3, 0.5, 0.7, 0.9, 0.99, 0.999999)))
    empty = {"Z": 0, "rim": 0, "nz": 0, "Sx": 0, "Sy": 0, "Sxx": 0, "Sxy": 0, "Syy": 0}
    cases.append(("empty", empty, [0] * pdf_ref.BINS, [0] * pdf_ref.BINS, 3, 4, LEVELS))
    # sums of two words: 2^30 nodes of full mass along a 65 536-node axis
    Z = 1 << 60
    big = {"Z": Z, "rim": (1 << 45) + 12345, "nz": 1 << 30, "Sx": -((1 << 76) + 987654321), "Sy": (1 << 75) + 1,
           "Sxx": (1 << 92) + (1 << 70) + 3, "Sxy": -((1 << 91) + 5), "Syy": (1 << 92) - 7}
    count, mass = [0] * pdf_ref.BINS, [0] * pdf_ref.BINS
    count[960], mass[960] = 1 << 29, 1 << 59
    count[928], mass[928] = 1 << 30, 1 << 59
    cases.append(("two_words", big, count, mass, 40000, 60000, LEVELS))
    return cases


@pytest.mark.parametrize("which", ["plain", "san"])
def test_finalisation_program_agrees_with_the_restatement_bit_for_bit(programs, which):
    cases, text = final_cases(), ""
    for _, s, count, mass, ix, iy, levels in cases:
        bins = [(k, count[k], mass[k]) for k in range(pdf_ref.BINS) if count[k]]
        text += "final " + " ".join(str(s[k]) for k in ("Z", "rim", "nz", "Sx", "Sy", "Sxx", "Sxy", "Syy")) + f" {ix} {iy} "
        text += " ".join(hx(GRID[q]) for q in (0, 1, 3, 4)) + f" {len(levels)} " + " ".join(hx(c) for c in levels)
        text += f" {len(bins)} " + " ".join(f"{k} {c} {m}" for k, c, m in bins) + "\n"
    lines = subprocess.run([programs[which]], input=text, capture_output=True, text=True, check=True).stdout.split("\n")
    for n, (name, s, count, mass, ix, iy, levels) in enumerate(cases):
        got = lines[n].split()
        assert got[0] == "final", (name, lines[n])
        o = pdf_ref.finalize(s, count, mass, ix, iy, GRID, levels)
        want = np.array([o["mean_x"], o["mean_y"]] + o["cov"] + o["ellipse"] + [o["area"], o["rim_fraction"]])
        have = np.array([unhx(v) for v in got[1:11]])
        assert np.array_equal(have, want, equal_nan=True), (name, have, want)
        assert [int(got[11]), int(got[12])] == [o["nz"], o["mass"]], name
        for k in range(len(levels)):
            q = got[13 + 4 * k:17 + 4 * k]
            assert int(q[0]) == o["level_count"][k], (name, k)
            have = np.array([unhx(v) for v in q[1:]])
            want = np.array([o["level_area"][k], o["level_fraction"][k], o["level_rho"][k]])
            assert np.array_equal(have, want, equal_nan=True), (name, k, have, want)
        if name == "empty":
            assert o["mass"] == 0 and all(c == 0 for c in o["level_count"]) and np.isnan(want).all() and np.isnan(o["mean_x"])
        if name == "top_bin":
            assert o["level_count"] == [1] * 4 and o["level_rho"] == [1.0] * 4 and o["level_fraction"] == [1.0] * 4
        if name == "two_words":
            assert o["level_count"][0] == 1 << 29 and o["level_count"][1] == 3 << 29 and np.isfinite(have).all()
            assert o["cov"][0] > 0 and abs(o["mean_x"] - (GRID[0] + (40000 - 65536.0 - 987654321 / 2.0 ** 60) * GRID[1])) < 1e-6
        if name == "tilted":
            assert o["cov"][1] > 0 and 0 < o["ellipse"][2] < np.pi / 2 and o["ellipse"][0] > o["ellipse"][1] > 0


@pytest.mark.parametrize("which", ["plain", "san"])
def test_density_mass_bin_and_quantum_programs(programs, which):
    rng = np.random.default_rng(9)
    obj = np.concatenate([rng.uniform(0.0, 60.0, 500), [0.0, np.inf, np.nan, 1e6, 41.5, 41.6]])
    obj0, sw, sigma = 0.25, 7.0, 1.3
    val = np.concatenate([rng.uniform(0.0, 0.8, 500), [0.8, 0.0, -np.inf, np.nan]])
    ms = np.concatenate([np.arange(1, 70), 2 ** np.arange(31), 2 ** np.arange(1, 31) - 1, rng.integers(1, 2 ** 30, 300)])
    us = np.concatenate([rng.random(200), [0.0, -0.0, np.nextafter(1.0, 0.0), 1.0, 2.0, -1.0, np.nan, 5e-324]])
    Zs = [1, 2, 1 << 30, (1 << 30) + 1, (1 << 53) + 1, (1 << 60) - 1, 12345678901234567]
    text = "".join(f"l2 {hx(v + obj0)} {hx(obj0)} {hx(sw)} {hx(sigma)}\n" for v in obj)
    powers = (1, 2, 7, 13, 21, 4096)
    text += "".join(f"edt {hx(v)} {hx(0.8)} {p}\n" for p in powers for v in val)
    text += "".join(f"edt {hx(v)} {hx(0.0)} 3\n" for v in val[-6:])
    text += "".join(f"bin {m}\n" for m in ms)
    text += "".join(f"quantum {hx(u)} {Z}\n" for Z in Zs for u in us)
    out = subprocess.run([programs[which]], input=text, capture_output=True, text=True, check=True).stdout.split("\n")
    k = 0
    rho = pdf_ref.density_l2(obj + obj0, obj0, sw, sigma)
    for r in rho:
        got = out[k].split()
        assert got[0] == "l2" and unhx(got[1]) == r and int(got[2]) == int(pdf_ref.masses(np.array([r]))[0]), (k, out[k], r)
        k += 1
    assert rho[500] == 1.0 and (rho[501:504] == 0.0).all() and rho[:500].min() > 0.0
    for p in powers:
        for r in pdf_ref.density_edt(val, 0.8, p):
            got = out[k].split()
            assert got[0] == "edt" and unhx(got[1]) == r and int(got[2]) == int(pdf_ref.masses(np.array([r]))[0]), (k, out[k], r)
            k += 1
    for _ in range(6):
        assert out[k].split()[1:] == ["0x0p+0", "0"], out[k]
        k += 1
    for m in ms:
        b = pdf_ref.bin_of(int(m))
        assert out[k].split() == ["bin", str(b), str(pdf_ref.bin_edge(b))], (m, out[k])
        k += 1
    for Z in Zs:
        for u in us:
            assert out[k].split() == ["quantum", str(pdf_ref.sample_quantum(u, Z))], (u, Z, out[k])
            k += 1
