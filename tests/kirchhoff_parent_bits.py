"""The cases of tests/golden/kirchhoff_parent_bits.npz: what the Kirchhoff kernels of the commit before the three kernel families
were folded into one migrate / model pair computed, bit for bit.  tools/record_kirchhoff_bits.py ran these cases on that commit
and wrote the file; test_gpu_kirchhoff_parent_bits.py runs them on today's tree and compares.  Since the fold, the tests "one
arrival without kmah is today's operator" and "degenerate cases are today's multi handle" compare a kernel with itself, and the
model is held to its matrix only to 1e-12: this file is what keeps "bit for bit" against the three old kernel texts.

Tables and geometry: the small random cases of kirchhoff_multi_ref / kirchhoff_aa_ref (960 nodes, 5 positions, 23 traces, 64
samples), and per family one trace long enough for the model's window loop to run twice.
  one    rtmi_kirchhoff_create: bins 0, 6 and 17 (17: the 128-lane block), each bare and with amp + w + holes; 4 099 samples.
  multi  rtmi_kirchhoff_create_multi: K = 1 .. 4, without and with kmah, bins 0 and 5; 2 051 samples with kmah (512 lanes).
  aa     rtmi_kirchhoff_create_aa: K = 1 and 2, three levels, without and with kmah; 700 samples with kmah (W = 4096 / 6 = 682).
In multi and aa, amp + w + holes are on in every other case, by the parity of K + kmah (+ bins): every kernel flag is on and off
with each of the others.

The file holds, per case, SHA-256 digests of the inputs (a changed generator is told apart from a changed kernel), of the image
and of the modelled channels, and contributing / pairs of both kernels and scale_exp.  Digests of the raw bytes, because the
arrays of all cases in full are several times the size a golden file may have; equal digests are equal bits.  The two bin-free
cases of the one-arrival handle are also stored in full: theirs is the route whose model kernel text changed the most."""
import hashlib

import numpy as np

import kirchhoff_aa_ref as KA
import kirchhoff_multi_ref as KM

HW3 = KA.HW8[:3]
STATS = ("migrate contributing", "migrate pairs", "model contributing", "model pairs", "scale_exp")


def cases():
    """-> {name: dict(family, karr, nbin, opts, kmah, N, nt, seed, full)}"""
    out = {}

    def add(family, karr, nbin, opts, kmah, N=KM.SM_N, nt=KM.SM_NT, full=False):
        name = f"{family} K{karr} bins{nbin} {'opts' if opts else 'bare'} {'kmah' if kmah else 'nokmah'} N{N} nt{nt}"
        out[name] = dict(family=family, karr=karr, nbin=nbin, opts=opts, kmah=kmah, N=N, nt=nt, seed=700 + len(out), full=full)

    for nbin in (0, 6, 17):
        for opts in (False, True):
            add("one", 1, nbin, opts, False, full=nbin == 0)
    add("one", 1, 0, True, False, N=1, nt=4099)
    for karr in (1, 2, 3, 4):
        for kmah in (False, True):
            for nbin in (0, 5):
                add("multi", karr, nbin, (karr + kmah + (nbin > 0)) % 2 == 0, kmah)
    add("multi", 2, 0, True, True, N=1, nt=2051)
    for karr in (1, 2):
        for kmah in (False, True):
            add("aa", karr, 5 if karr == 2 else 0, (karr + kmah) % 2 == 0, kmah)
    add("aa", 2, 0, True, True, N=1, nt=700)
    return out


def digest(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        if a is None:
            h.update(b"none;")
            continue
        a = np.ascontiguousarray(a)
        h.update(f"{a.dtype.str}{a.shape};".encode())
        h.update(a.tobytes())
    return h.hexdigest()


def run(rb, c):
    """One case on the device -> dict(inputs, image, channels, stats): the digest of everything the operator and its two calls
    were given, the image, the modelled channels [1 or 2, N, nt] and the five integers of STATS."""
    o, kmah, nbin, nt = c["opts"], c["kmah"], c["nbin"], c["nt"]
    pt = aa = None
    if c["family"] == "aa":
        T, pt, aa, isrc, irec, kw = KA.small_case(c["karr"], hw=HW3, pt_holes=o, nbin=nbin, amp=o, w=o, kmah=kmah, holes=o, seed=c["seed"],
                                                  N=c["N"], nt=nt)
    else:
        T, isrc, irec, kw = KM.small_case(c["karr"], nbin, o, o, kmah, o, seed=c["seed"], N=c["N"], nt=nt)
    rng = np.random.default_rng(c["seed"])
    d0, d1 = rng.standard_normal((2, len(isrc), nt))
    m = rng.standard_normal((max(nbin, 1),) + T.shape[2:])
    inputs = digest(T, pt, None if aa is None else np.array(aa["hw"] + (aa["asrc"], aa["arec"], aa["amid"]), dtype=np.float64), isrc, irec,
                    kw["amp"], kw["theta"], kw["kmah"], kw["w"], np.array([nbin, kw["dopen"] or 0.0, KM.SM_DT]), d0, d1, m)
    common = dict(weights=kw["w"], nbin=nbin, dopen=kw["dopen"])
    if c["family"] == "one":
        first = lambda a: None if a is None else a[:, 0]             # noqa: E731
        op = rb.Kirchhoff(T[:, 0], isrc, irec, nt, KM.SM_DT, amp=first(kw["amp"]), theta=first(kw["theta"]), **common)
        img, st = op.migrate(d0, stats=True)
        ch, sm = op.model(m, stats=True)
        ch = ch[None]
    else:
        op = rb.Kirchhoff(T, isrc, irec, nt, KM.SM_DT, amp=kw["amp"], theta=kw["theta"], kmah=kw["kmah"], pt=pt, antialias=aa, **common)
        img, st = op.migrate_channels(d0, d1 if kmah else None, stats=True)
        (c0, c1), sm = op.model_channels(m, stats=True)
        ch = np.stack([c0, c1]) if kmah else c0[None]
        assert kmah or not np.any(c1)
    op.close()
    stats = np.array([st["contributing"], st["pairs"], sm["contributing"], sm["pairs"], sm["scale_exp"]], dtype=np.int64)
    assert 0 < stats[0] < stats[1], "a case in which every pair or none contributes checks little"
    return dict(inputs=inputs, image=np.asarray(img), channels=np.asarray(ch), stats=stats)
