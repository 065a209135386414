"""Ungapped (Hamming) scoring on the device: nvbio_hip_hamming_score / _qual / _qual_jobs (nvbio_amd/csrc/hamming.hip) against the model of
tests/test_hamming_host.py on its matrix of shapes, against the host twin on larger batches, and through the Python host layer."""
import ctypes as C

import numpy as np
import pytest
import torch

import nvbio_amd as nvb
from nvbio_amd import _lib
from oracle import pyoracle as O
from tests import test_hamming_host as H

pytestmark = pytest.mark.gpu
GLOBAL, LOCAL, SEMI = 0, 1, 2
KERNEL = b"hamming_score_kernel"


def dev_set(hs, fixed_length=None):
    return nvb.PackedStringSet.from_host(hs.words, hs.bits, hs.big_endian, hs.begin, hs.length if fixed_length is None else None,
                                         fixed_length or 0, device="cuda")


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def run_device(hp, ht, qcat, match, lut, flat, typ, ms, fixed=None, max_m=None, max_n=None, jobs=None, algorithm=0, expect=0):
    """one call of the device entry; jobs = (n_on_device, job_index, gate, gate_limit, wave_form) for the job-control form"""
    L = nvb.lib()
    n = len(hp)
    dp, dt = dev_set(hp, None if fixed is None else fixed[0]), dev_set(ht, None if fixed is None else fixed[1])
    sp, st = dp.struct(), dt.struct()
    max_m = int(hp.length.max()) if max_m is None else max_m
    max_n = int(ht.length.max()) if max_n is None else max_n
    score = torch.full((n,), 77, dtype=torch.int32, device="cuda"); sink = torch.full((n, 2), 77, dtype=torch.int32, device="cuda")
    ok = torch.full((n,), 77, dtype=torch.uint8, device="cuda")
    dms = None if ms is None else dev(ms)
    msp = None if ms is None else C.c_void_p(dms.data_ptr())
    out = (C.c_void_p(score.data_ptr()), C.c_void_p(sink.data_ptr()), C.c_void_p(ok.data_ptr()), None)
    if lut is None:
        sc = _lib.GotohSchemeStruct(match, flat, -1000, -1000)
        e = L.nvbio_hip_hamming_score(C.byref(sc), algorithm, typ, C.byref(sp), C.byref(st), max_m, max_n, msp, n, *out)
    else:
        sc = H.qual_struct(match, lut)
        dq = dev(qcat)
        if jobs is None:
            e = L.nvbio_hip_hamming_score_qual(C.byref(sc), algorithm, typ, C.byref(sp), C.c_void_p(dq.data_ptr()), dq.numel(), C.byref(st), max_m, max_n, msp, n, *out)
        else:
            n_dev, index, gate, limit, wave = jobs
            keep = [dev(np.array([n_dev], np.uint32).view(np.int32)), dev(index.astype(np.uint32).view(np.int32)), dev(np.array([gate], np.uint32).view(np.int32))]
            e = L.nvbio_hip_hamming_score_qual_jobs(C.byref(sc), algorithm, typ, C.byref(sp), C.c_void_p(dq.data_ptr()), dq.numel(), C.byref(st), max_m, max_n, msp, n,
                                                    C.c_void_p(keep[0].data_ptr()), C.c_void_p(keep[1].data_ptr()), C.c_void_p(keep[2].data_ptr()), limit, wave, *out)
    assert e == expect, e
    torch.cuda.synchronize()
    return ok.cpu().numpy(), score.cpu().numpy(), sink.cpu().numpy().view(np.uint32)


def run_case(c, qual, typ, ms, **kw):
    match, lut, flat = H.scheme_of(qual, typ)
    return run_device(c["hp"], c["ht"], c["qcat"], match, lut, flat, typ, ms, fixed=c["fixed"], **kw)


@pytest.mark.parametrize("typ", [GLOBAL, LOCAL, SEMI])
@pytest.mark.parametrize("qual", H.QUALS)
@pytest.mark.parametrize("fmt", list(H.FORMATS))
def test_device_matrix(fmt, qual, typ):
    """every shape of the matrix (block, word and wave edges, texts shorter than the pattern, empty texts), four kinds of threshold"""
    c, exp = H.make_case(fmt, qual), H.expected(fmt, qual, typ)
    H.assert_thresholds_bind(exp)
    for kind, want in exp.items():
        H.check(run_case(c, qual, typ, want[0]), want, "%s %s type %d min_score %s" % (fmt, qual, typ, kind))
    assert nvb.lib().nvbio_hip_last_kernel() == KERNEL


@pytest.mark.parametrize("typ", [GLOBAL, LOCAL, SEMI])
@pytest.mark.parametrize("shape", [(17, 1), (64, 64), (150, 333)])
def test_device_fixed_length(shape, typ):
    c, exp = H.make_case("4bit", "phred", 5, shape), H.expected("4bit", "phred", typ, 5, shape)
    for kind, want in exp.items():
        H.check(run_case(c, "phred", typ, want[0], max_m=shape[0], max_n=shape[1]), want, "fixed %s type %d min_score %s" % (shape, typ, kind))


@pytest.mark.parametrize("typ", [GLOBAL, LOCAL, SEMI])
def test_device_beyond_int16(typ):
    """costs that take the values past int16: the column between two blocks keeps their low 16 bits, as the reference's does"""
    c, want = H.wide_case(typ)
    H.check(run_device(c["hp"], c["ht"], None, H.WIDE["match"], None, H.WIDE["flat"], typ, None), want, "wide type %d" % typ)


def big_batch(seed, n, max_m, max_n, fmt="4bit"):
    bits, pbe, tbe, sigma, odd = H.FORMATS[fmt]
    rng = np.random.default_rng(seed)
    pats, texts = [], []
    for i in range(n):
        M, N = int(rng.integers(1, max_m + 1)), int(rng.integers(0, max_n + 1))
        p = rng.integers(0, sigma, M).astype(np.uint8)
        t = rng.integers(0, sigma, N).astype(np.uint8)
        if i % 3 and N >= M:
            off = int(rng.integers(0, N - M + 1))
            t[off:off + M] = p
            for _ in range(int(rng.integers(0, 6))):
                t[off + int(rng.integers(0, M))] = rng.integers(0, sigma)
        if i % 7 == 0:
            p[int(rng.integers(0, M))] = 4
        pats.append(p); texts.append(t)
    quals = [rng.integers(2, 41, len(p)).astype(np.uint8) for p in pats]
    return O.StringSet.from_lists(pats, bits, pbe), O.StringSet.from_lists(texts, 2, tbe), np.concatenate(quals)


def host_twin(hp, ht, qcat, match, lut, typ, ms):
    n = len(hp)
    sp, st = H.sset(hp), H.sset(ht)
    score = np.zeros(n, np.int32); sink = np.zeros((n, 2), np.uint32); ok = np.zeros(n, np.uint8)
    sc = H.qual_struct(match, lut)
    assert nvb.lib().nvbio_hip_hamming_score_qual_host(C.byref(sc), 0, typ, C.byref(sp), qcat.ctypes.data, qcat.size, C.byref(st),
                                                       None if ms is None else ms.ctypes.data, n, score.ctypes.data, sink.ctypes.data, ok.ctypes.data, 0) == 0
    return ok, score, sink


@pytest.mark.parametrize("typ", [GLOBAL, LOCAL, SEMI])
def test_device_against_host_twin(typ):
    """4000 ragged jobs up to 200 x 700 (twelve passes of 64 rows, thirteen blocks); per-job thresholds, half of them around the job's own
    best, half where the first blocks' edges lie"""
    hp, ht, qcat = big_batch(40 + typ, 4000, 200, 700)
    match, lut, _ = H.scheme_of("phred", typ)
    free = host_twin(hp, ht, qcat, match, lut, typ, None)
    H.check(run_device(hp, ht, qcat, match, lut, 0, typ, None), (None,) + free, "null")
    rng = np.random.default_rng(3)
    ms = (free[1].astype(np.int64) + rng.integers(-3, 2, len(hp))).clip(-(1 << 30), None)
    ms = np.where(rng.random(len(hp)) < 0.5, ms, rng.integers(-40, 41, len(hp))).astype(np.int32)
    want = host_twin(hp, ht, qcat, match, lut, typ, ms)
    assert 0.05 * len(hp) < int(want[0].sum()) < 0.95 * len(hp)                       # both outcomes of the early exit occur
    H.check(run_device(hp, ht, qcat, match, lut, 0, typ, ms), (ms,) + want, "thresholds")


@pytest.mark.parametrize("typ", [LOCAL, SEMI])
def test_job_list_form(typ):
    """the job-control entry: the gated whole batch, and a list of jobs run in place, against the plain form"""
    hp, ht, qcat = big_batch(50 + typ, 3000, 160, 400)
    match, lut, _ = H.scheme_of("phred", typ)
    n = len(hp)
    ms = np.full(n, -60, np.int32)
    plain = run_device(hp, ht, qcat, match, lut, 0, typ, ms)
    # wave_form = 0 runs when *gate > gate_limit
    got = run_device(hp, ht, qcat, match, lut, 0, typ, ms, jobs=(0, np.zeros(1), 10, 5, 0))
    H.check(got, (ms,) + plain, "gated, open")
    closed = run_device(hp, ht, qcat, match, lut, 0, typ, ms, jobs=(0, np.zeros(1), 5, 5, 0))
    assert (closed[1] == 77).all() and (closed[0] == 77).all()
    # wave_form = 1: a list of 700 jobs, of which the device-side count admits 500; runs when *gate <= gate_limit
    index = np.random.default_rng(9).permutation(n)[:700]
    got = run_device(hp, ht, qcat, match, lut, 0, typ, ms, jobs=(500, index, 5, 5, 1))
    sel = np.zeros(n, bool); sel[index[:500]] = True
    assert (got[0][sel] == plain[0][sel]).all() and (got[1][sel] == plain[1][sel]).all() and (got[2][sel] == plain[2][sel]).all()
    assert (got[1][~sel] == 77).all() and (got[0][~sel] == 77).all() and (got[2][~sel] == 77).all()
    closed = run_device(hp, ht, qcat, match, lut, 0, typ, ms, jobs=(500, index, 6, 5, 1))
    assert (closed[1] == 77).all()


@pytest.mark.parametrize("typ", [GLOBAL, LOCAL, SEMI])
def test_python_layer(typ):
    """batch_alignment_score(make_hamming_distance_aligner(...)) over a simple scheme and over nvBowtie's scheme with qualities"""
    c = H.make_case("4bit", "simple")
    exp = H.expected("4bit", "simple", typ)["best"]
    match, _, flat = H.scheme_of("simple", typ)
    al = nvb.make_hamming_distance_aligner(typ, nvb.SimpleSmithWatermanScheme(match, flat, -9, -9))
    dp, dt = dev_set(c["hp"]), dev_set(c["ht"])
    score, sink, ok = nvb.batch_alignment_score(al, dp, dt, 150, 333, min_score=dev(exp[0]))
    H.check((ok.cpu().numpy(), score.cpu().numpy(), sink.cpu().numpy().view(np.uint32)), exp, "python, simple scheme")
    # nvBowtie's scheme: its own table of penalties by quality
    scheme = nvb.SmithWatermanScoringScheme.local() if typ == LOCAL else nvb.SmithWatermanScoringScheme()
    lut = np.array([scheme.mismatch(q) for q in range(256)], np.int32)
    hp, ht, qcat = big_batch(60 + typ, 1500, 150, 400)
    want = host_twin(hp, ht, qcat, scheme.match(), lut, typ, None)
    al = nvb.make_hamming_distance_aligner(typ, scheme)
    score, sink, ok = nvb.batch_alignment_score(al, dev_set(hp), dev_set(ht), 150, 400, quals=dev(qcat))
    H.check((ok.cpu().numpy(), score.cpu().numpy(), sink.cpu().numpy().view(np.uint32)), (None,) + want, "python, quality scheme")
    assert nvb.lib().nvbio_hip_last_kernel() == KERNEL


def test_limits():
    """the stated limits: 1024-symbol patterns on 65535-symbol texts run (and agree with the host twin); text blocking, patterns past 4096
    symbols, costs past 2^20 and a working set past the LDS are refused with hipErrorNotSupported, before anything is launched"""
    rng = np.random.default_rng(77)
    pats = [rng.integers(0, 4, 1024).astype(np.uint8), rng.integers(0, 4, 1000).astype(np.uint8), rng.integers(0, 4, 33).astype(np.uint8)]
    texts = [rng.integers(0, 4, 65535).astype(np.uint8), rng.integers(0, 4, 40000).astype(np.uint8), rng.integers(0, 4, 65535).astype(np.uint8)]
    texts[0][60000:61024] = pats[0]; texts[0][60010] ^= 1
    texts[1][39000:40000] = pats[1]
    hp, ht = O.StringSet.from_lists(pats, 4, True), O.StringSet.from_lists(texts, 2, False)
    qcat = rng.integers(2, 41, sum(len(p) for p in pats)).astype(np.uint8)
    for typ in (LOCAL, SEMI, GLOBAL):
        match, lut, _ = H.scheme_of("phred", typ)
        want = host_twin(hp, ht, qcat, match, lut, typ, None)
        H.check(run_device(hp, ht, qcat, match, lut, 0, typ, None, max_m=1024, max_n=65535), (None,) + want, "1024 x 65535, type %d" % typ)
    match, lut, _ = H.scheme_of("phred", SEMI)
    small_p, small_t, small_q = big_batch(1, 50, 40, 80)
    run_device(small_p, small_t, small_q, match, lut, 0, SEMI, None, algorithm=1, expect=801)
    run_device(small_p, small_t, small_q, match, lut, 0, SEMI, None, max_m=4097, expect=801)
    run_device(small_p, small_t, small_q, match, lut, 0, SEMI, None, max_n=1 << 20, expect=801)
    run_device(small_p, small_t, small_q, (1 << 20) + 1, lut, 0, SEMI, None, expect=801)
    n = len(small_p)                                                                         # the limit itself runs
    sp, st = H.sset(small_p), H.sset(small_t)
    score = np.zeros(n, np.int32); sink = np.zeros((n, 2), np.uint32); ok = np.zeros(n, np.uint8)
    sc = _lib.GotohSchemeStruct(1 << 20, -(1 << 20), 0, 0)
    for typ in (LOCAL, SEMI):
        assert nvb.lib().nvbio_hip_hamming_score_host(C.byref(sc), 0, typ, C.byref(sp), C.byref(st), None, n, score.ctypes.data, sink.ctypes.data, ok.ctypes.data, 0) == 0
        H.check(run_device(small_p, small_t, small_q, 1 << 20, None, -(1 << 20), typ, None), (None, ok, score, sink), "costs of 2^20, type %d" % typ)
    run_device(small_p, small_t, small_q, 1, None, -(1 << 20) - 1, SEMI, None, expect=801)


# ------------------------------------------------------------------------------------------------ the C++ host layer
def cxx_lib(name):
    import os
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), *name)
    assert os.path.exists(path), "build() compiles %s" % path
    return C.CDLL(path)


@pytest.mark.parametrize("typ", [GLOBAL, LOCAL, SEMI])
def test_cxx_host_class(typ):
    """aln::HammingDistanceAligner through aln::batch_alignment_score / BatchedAlignmentScore (include/nvbio_hip/alignment.h)"""
    shim = cxx_lib(("cxx", "libhamming_shim.so"))
    c = H.make_case("4bit", "simple")
    exp = H.expected("4bit", "simple", typ)
    match, _, flat = H.scheme_of("simple", typ)
    n = len(c["pats"])
    dp, dt = dev_set(c["hp"]), dev_set(c["ht"])
    sp, st = dp.struct(), dt.struct()
    for kind in ("null", "best"):
        want = exp[kind]
        score = torch.full((n,), 77, dtype=torch.int32, device="cuda"); sink = torch.full((n, 2), 77, dtype=torch.int32, device="cuda")
        ok = torch.full((n,), 77, dtype=torch.uint8, device="cuda")
        dms = None if want[0] is None else dev(want[0])
        assert shim.hamming_host_class(typ, match, flat, 0, 0, 0, C.byref(sp), None, C.c_uint64(0), C.byref(st), n, 150, 333,
                                       None if dms is None else C.c_void_p(dms.data_ptr()), C.c_void_p(score.data_ptr()), C.c_void_p(sink.data_ptr()),
                                       None if dms is None else C.c_void_p(ok.data_ptr())) == 0
        torch.cuda.synchronize()
        got_ok = ok.cpu().numpy() if dms is not None else want[1]           # the plain batch function has no ok array
        H.check((got_ok, score.cpu().numpy(), sink.cpu().numpy().view(np.uint32)), want, "C++ host class, simple scheme, %s" % kind)
    # nvBowtie's scheme with the reads' quality bytes
    hp, ht, qcat = big_batch(70 + typ, 1500, 150, 400)
    scheme = nvb.SmithWatermanScoringScheme.local() if typ == LOCAL else nvb.SmithWatermanScoringScheme()
    lut = np.array([scheme.mismatch(q) for q in range(256)], np.int32)
    ms = np.full(len(hp), -30, np.int32)
    want = host_twin(hp, ht, qcat, scheme.match(), lut, typ, ms)
    dp, dt, dq, dms = dev_set(hp), dev_set(ht), dev(qcat), dev(ms)
    sp, st = dp.struct(), dt.struct()
    n = len(hp)
    score = torch.zeros(n, dtype=torch.int32, device="cuda"); sink = torch.zeros((n, 2), dtype=torch.int32, device="cuda"); ok = torch.zeros(n, dtype=torch.uint8, device="cuda")
    assert shim.hamming_host_class(typ, scheme.match(), 0, 1, 2, 6, C.byref(sp), C.c_void_p(dq.data_ptr()), C.c_uint64(dq.numel()), C.byref(st), n, 150, 400,
                                   C.c_void_p(dms.data_ptr()), C.c_void_p(score.data_ptr()), C.c_void_p(sink.data_ptr()), C.c_void_p(ok.data_ptr())) == 0
    torch.cuda.synchronize()
    H.check((ok.cpu().numpy(), score.cpu().numpy(), sink.cpu().numpy().view(np.uint32)), (ms,) + want, "C++ host class, quality scheme")


# ------------------------------------------------------------------------------------------------ the drop-in layer
def offsets32(hs):
    return np.concatenate([hs.begin, [int(hs.begin[-1]) + int(hs.length[-1])]]).astype(np.uint32)


def layer_packed(lib, typ, text_blocking, match, flat, hp, ht, ms):
    n = len(hp)
    keep = [dev(offsets32(hp).view(np.int32)), dev(hp.words.view(np.int32)), dev(offsets32(ht).view(np.int32)), dev(ht.words.view(np.int32))]
    dms = None if ms is None else dev(ms)
    score = torch.full((n,), 77, dtype=torch.int32, device="cuda"); sink = torch.full((n, 2), 77, dtype=torch.int32, device="cuda")
    path = C.create_string_buffer(16)
    assert lib.hamming_packed(typ, text_blocking, match, flat, n, C.c_void_p(keep[0].data_ptr()), C.c_void_p(keep[1].data_ptr()), int(hp.length.max()),
                              C.c_void_p(keep[2].data_ptr()), C.c_void_p(keep[3].data_ptr()), int(ht.length.max()),
                              None if dms is None else C.c_void_p(dms.data_ptr()), C.c_void_p(score.data_ptr()), C.c_void_p(sink.data_ptr()), path) == 0
    return path.value, score.cpu().numpy(), sink.cpu().numpy().view(np.uint32)


@pytest.mark.parametrize("typ", [GLOBAL, LOCAL, SEMI])
def test_layer_packed_stream(typ, monkeypatch):
    """BatchedAlignmentScore over a zero-copy packed stream: the tuned kernel by default, the generic lane under NVBIO_HIP_COMPAT_GENERIC=full
    and for TextBlockingTag; the same sinks on both lanes, and the model's"""
    lib = cxx_lib(("compat", "libhamming_callers.so"))
    c = H.make_case("4bit", "simple")
    exp = H.expected("4bit", "simple", typ)
    match, _, flat = H.scheme_of("simple", typ)
    for kind in ("null", "best"):
        ms, eok, escore, esink = exp[kind]
        monkeypatch.delenv("NVBIO_HIP_COMPAT_GENERIC", raising=False)
        path, score, sink = layer_packed(lib, typ, 0, match, flat, c["hp"], c["ht"], ms)
        assert path == b"tuned" and nvb.lib().nvbio_hip_last_kernel() == KERNEL
        monkeypatch.setenv("NVBIO_HIP_COMPAT_GENERIC", "full")
        gpath, gscore, gsink = layer_packed(lib, typ, 0, match, flat, c["hp"], c["ht"], ms)
        assert gpath == b"generic"
        assert (score == gscore).all() and (sink == gsink).all()
        assert (score == escore).all() and (sink == esink).all()
    # TextBlockingTag: the ABI refuses it (test_limits), the layer keeps the stream on the generic lane; LOCAL scores are order-free
    monkeypatch.delenv("NVBIO_HIP_COMPAT_GENERIC", raising=False)
    tpath, tscore, _ = layer_packed(lib, typ, 1, match, flat, c["hp"], c["ht"], None)
    assert tpath == b"generic"
    if typ == LOCAL:
        assert (tscore == exp["null"][2]).all()


def test_layer_over_limit_shape(monkeypatch):
    """patterns beyond the kernel's 4096 symbols: the entry answers 801 and the layer scores the batch on its generic lane"""
    lib = cxx_lib(("compat", "libhamming_callers.so"))
    rng = np.random.default_rng(5)
    pats = [rng.integers(0, 4, m).astype(np.uint8) for m in (5000, 4097, 20)]
    texts = [rng.integers(0, 4, m).astype(np.uint8) for m in (5200, 3000, 50)]
    texts[0][100:5100] = pats[0]; texts[0][777] ^= 1
    hp, ht = O.StringSet.from_lists(pats, 4, True), O.StringSet.from_lists(texts, 2, False)
    sp, st = H.sset(hp), H.sset(ht)
    score = np.zeros(3, np.int32); sink = np.zeros((3, 2), np.uint32); ok = np.zeros(3, np.uint8)
    sc = _lib.GotohSchemeStruct(2, -3, 0, 0)
    assert nvb.lib().nvbio_hip_hamming_score_host(C.byref(sc), 0, SEMI, C.byref(sp), C.byref(st), None, 3, score.ctypes.data, sink.ctypes.data, ok.ctypes.data, 0) == 0
    monkeypatch.delenv("NVBIO_HIP_COMPAT_GENERIC", raising=False)
    path, gscore, gsink = layer_packed(lib, SEMI, 0, 2, -3, hp, ht, None)
    assert path == b"generic" and (gscore == score).all() and (gsink == sink).all()


def pack_be(sym, bits):
    per = 32 // bits
    pad = np.zeros((-len(sym)) % per + 4 * per, np.uint8)
    v = np.concatenate([sym, pad]).astype(np.uint32).reshape(-1, per)
    sh = (32 - bits - bits * np.arange(per)).astype(np.uint32)
    return (v << sh).sum(axis=1).astype(np.uint32)


@pytest.mark.parametrize("typ", [LOCAL, SEMI])
def test_layer_read_views_with_qualities(typ, monkeypatch):
    """a stream shaped like nvBowtie's opposite-mate stream under --ungapped-mates: io::ReadStream views (forward / reverse complement) with
    their quality strings, a scheme of nvBowtie's concept, genome windows, thresholds, some jobs declined by init_context"""
    lib = cxx_lib(("compat", "libhamming_callers.so"))
    rng = np.random.default_rng(21 + typ)
    n, G = 3000, 1 << 16
    genome = rng.integers(0, 4, G).astype(np.uint8)
    lens = rng.integers(20, 151, n)
    offs = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint32)
    reads = np.zeros(int(offs[-1]), np.uint8)
    windows = np.zeros((n, 2), np.uint32)
    for i in range(n):
        L = int(lens[i]); lo = int(rng.integers(0, G - 700)); span = int(rng.integers(L, 650)) if i % 11 else 0
        windows[i] = (lo, lo + span)
        at = lo + int(rng.integers(0, max(span - L, 0) + 1))
        r = genome[at:at + L].copy() if i % 4 else rng.integers(0, 4, L).astype(np.uint8)
        for _ in range(int(rng.integers(0, 5))):
            r[int(rng.integers(0, L))] = rng.integers(0, 5)
        reads[offs[i]:offs[i + 1]] = r
    quals = rng.integers(2, 41, reads.size).astype(np.uint8)
    match = 2 if typ == LOCAL else 0
    ms = rng.integers(-40, 10, n).astype(np.int32) + (match * lens).astype(np.int32)
    keep = [dev(offs.view(np.int32)), dev(pack_be(reads, 4).view(np.int32)), dev(quals), dev(pack_be(genome, 2).view(np.int32)), dev(windows.view(np.int32)), dev(ms)]

    def run():
        score = torch.full((n,), 77, dtype=torch.int32, device="cuda"); sink = torch.full((n, 2), 77, dtype=torch.int32, device="cuda")
        path = C.create_string_buffer(16)
        assert lib.hamming_views(typ, 1, match, 2, 6, n, C.c_void_p(keep[0].data_ptr()), C.c_void_p(keep[1].data_ptr()), C.c_void_p(keep[2].data_ptr()), 150,
                                 C.c_void_p(keep[3].data_ptr()), C.c_void_p(keep[4].data_ptr()), 650, C.c_void_p(keep[5].data_ptr()),
                                 C.c_void_p(score.data_ptr()), C.c_void_p(sink.data_ptr()), path) == 0
        return path.value, score.cpu().numpy(), sink.cpu().numpy().view(np.uint32)
    monkeypatch.delenv("NVBIO_HIP_COMPAT_GENERIC", raising=False)
    path, score, sink = run()
    assert path == b"tuned" and nvb.lib().nvbio_hip_last_kernel() == KERNEL
    monkeypatch.setenv("NVBIO_HIP_COMPAT_GENERIC", "full")
    gpath, gscore, gsink = run()
    assert gpath == b"generic"
    assert (score == gscore).all() and (sink == gsink).all()
    # the forward jobs against the host twin: pattern = the stored read, text = the genome window
    fwd = [i for i in range(0, n, 2)]
    hp = O.StringSet.from_lists([reads[offs[i]:offs[i + 1]] for i in fwd], 4, True)
    ht = O.StringSet.from_lists([genome[windows[i, 0]:windows[i, 1]] for i in fwd], 2, False)
    lut = np.array([-(2 + int(np.float32(np.float32(min(q, 40)) / np.float32(40.0)) * np.float32(4))) for q in range(256)], np.int32)
    _, wscore, wsink = host_twin(hp, ht, np.concatenate([quals[offs[i]:offs[i + 1]] for i in fwd]), match, lut, typ, ms[fwd])
    looked = windows[fwd, 1] > windows[fwd, 0]
    assert (score[fwd][looked] == wscore[looked]).all() and (sink[fwd][looked] == wsink[looked]).all()
    assert (score[fwd][~looked] == -(1 << 30)).all() and (~looked).sum() > 50
