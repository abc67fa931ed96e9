"""GPU: the one migrate / model kernel pair against the recorded bits of the three kernel families it replaced
(tests/golden/kirchhoff_parent_bits.npz, written by tools/record_kirchhoff_bits.py on the commit before the fold): images,
modelled channels, counts and scale_exp, equal bit for bit.  The cases and what the file holds: tests/kirchhoff_parent_bits.py."""
import ctypes as C
import os

import numpy as np
import pytest

import kirchhoff_parent_bits as PB

pytestmark = pytest.mark.gpu

CASES = PB.cases()


@pytest.fixture(scope="module")
def rb():
    from raytracing_amd import rt_bench, _lib
    n = C.c_int()
    _lib.check(_lib.lib().rtmi_device_count(n))
    assert n.value >= 1, "no HIP device"
    return rt_bench


@pytest.fixture(scope="module")
def recorded():
    with np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "kirchhoff_parent_bits.npz")) as z:
        return {k: z[k] for k in z.files}


def test_the_file_holds_exactly_these_cases(recorded):
    assert {k.rsplit("/", 1)[0] for k in recorded} == set(CASES)


@pytest.mark.parametrize("name", list(CASES))
def test_bits_of_the_three_kernel_families(rb, recorded, name):
    c = CASES[name]
    r = PB.run(rb, c)
    assert r["inputs"] == str(recorded[f"{name}/inputs"]), "the case's inputs are not the recorded ones: the generator changed, not the kernel"
    got = dict(zip(PB.STATS, r["stats"].tolist()))
    print(f"{name}: {got}")
    assert got == dict(zip(PB.STATS, recorded[f"{name}/stats"].tolist()))
    if c["full"]:
        assert np.array_equal(r["image"], recorded[f"{name}/image"]), f"{np.max(np.abs(r['image'] - recorded[f'{name}/image'])):.3e}"
        assert np.array_equal(r["channels"], recorded[f"{name}/channels"]), f"{np.max(np.abs(r['channels'] - recorded[f'{name}/channels'])):.3e}"
    assert PB.digest(r["image"]) == str(recorded[f"{name}/image_sha256"]), "the image differs from the recorded one"
    assert PB.digest(r["channels"]) == str(recorded[f"{name}/channels_sha256"]), "the modelled channels differ from the recorded ones"
