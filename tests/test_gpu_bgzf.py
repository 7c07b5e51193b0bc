"""The device BGZF inflater (sfgpu_bgzf_inflate_host, sailfish_amd/csrc/bgzf_read.hip) against the serial run of the same
contract header (tests/bgzf_harness.cpp) in everything it reports; the parser's device-text entry (sfgpu_reads_parse_device)
against sfgpu_reads_parse_host; then the file driver (readfile.ReadFile on a BGZF file) against the same text as a plain file,
and quantify_files end to end."""
import ctypes as C
import gzip
import os

import numpy as np
import pytest

from test_bgzf_cpu import (CRC_MISMATCH, ERR_FORMAT, NONE, OK, ROUND_TRIP_NAMES, TRUNCATED, Harness, build_harness,
                           error_members, hand_members, round_trip_files, text_3000, unpack)
from test_gpu_readfile import SHAPES, _render, _sample
from test_readfile_cpu import fastq_text


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    return Harness(build_harness(tmp_path_factory.mktemp("bgzh")))


@pytest.fixture(scope="module")
def files():
    return round_trip_files()


def device_inflate(gpu, data, final=1, cap=None, n_bytes=None, offset=0):
    """sfgpu_bgzf_inflate_host as Harness.inflate reports; the payload is written `offset` bytes into a guarded buffer"""
    import torch
    from sailfish_amd import _lib
    data = bytes(data)
    n = len(data) if n_bytes is None else n_bytes
    room = 65536 * (n // 26 + 1) if cap is None else cap
    size = min(room, 1 << 28)
    out = torch.full((offset + size + 64,), 0xA5, dtype=torch.uint8, device=gpu)
    res = _lib.BgzfResult()
    with torch.cuda.device(gpu):
        rc = _lib.lib().sfgpu_bgzf_inflate_host(data, n, int(final), _lib.ptr(out[offset:]), room, C.byref(res), _lib.current_stream_ptr())
    assert res.ms_copy >= 0 and res.ms_kernels >= 0
    host = out.cpu().numpy()
    if rc == OK:                        # nothing outside [0, n_bytes_out) was touched
        assert (host[:offset] == 0xA5).all() and (host[offset + res.n_bytes_out:] == 0xA5).all()
    return unpack(rc, res, host[offset:])


def same(got, want, what=""):
    for k in ("rc", "out", "n_members", "consumed", "n_bytes_out", "blocks", "error"):
        assert got[k] == want[k], (k, got[k] if k != "out" else len(got[k]), want[k] if k != "out" else len(want[k]), what)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ROUND_TRIP_NAMES)
def test_inflate_equals_the_harness(gpu, harness, files, name):
    data, payload, _, _ = files[name]
    want = harness.inflate(data)
    got = device_inflate(gpu, data)
    same(got, want, name)
    assert got["rc"] == OK and got["out"] == payload


@pytest.mark.gpu
def test_hand_assembled_and_concatenated(gpu, harness, files):
    from sailfish_amd import gzfile
    hand = hand_members()
    for name, (member, payload) in hand.items():
        got = device_inflate(gpu, member)
        same(got, harness.inflate(member), name)
        assert got["out"] == payload and got["blocks"] == (0, 1, 0)
    # one file of everything: members of every layout, an empty member in the middle, the EOF member at the end; written 5
    # bytes into the buffer (the payload need not be aligned)
    parts = [files[n][0][: -len(gzfile.BGZF_EOF)] for n in ("level6", "level0", "fixed", "full_flush_20001", "random_65000")]
    parts.insert(2, gzfile.BGZF_EOF)
    data = b"".join(parts) + b"".join(m for m, _ in hand.values()) + gzfile.BGZF_EOF
    want = harness.inflate(data)
    got = device_inflate(gpu, data, offset=5)
    same(got, want, "concatenated")
    assert got["rc"] == OK and got["out"] == gzip.decompress(data) and got["n_members"] > 30 and got["consumed"] == len(data)


@pytest.mark.gpu
def test_partial_input_and_capacity(gpu, harness, files):
    data, payload, _, _ = files["level6"]
    first = int.from_bytes(data[16:18], "little") + 1
    second = first + int.from_bytes(data[first + 16:first + 18], "little") + 1
    for cut in (second - 1, second + 17, second + 30, first + 5, 11):
        want = harness.inflate(data, final=0, n_bytes=cut)
        got = device_inflate(gpu, data, final=0, n_bytes=cut)
        same(got, want, cut)
        assert got["rc"] == OK and got["consumed"] == (0 if cut < first else first if cut < second else second)
        assert got["out"] == payload[: 65280 * got["n_members"]]
        want = harness.inflate(data, final=1, n_bytes=cut)
        got = device_inflate(gpu, data, final=1, n_bytes=cut)
        same(got, want, cut)
        assert got["rc"] == ERR_FORMAT and got["error"] == (TRUNCATED, want["n_members"])
    for cap in (2 * 65280 - 1, 2 * 65280, 0):
        want = harness.inflate(data, cap=cap)
        got = device_inflate(gpu, data, cap=cap)
        same(got, want, cap)
        assert got["rc"] == OK and got["n_members"] == cap // 65280 and got["out"] == payload[: 65280 * (cap // 65280)]
    # sizing only
    from sailfish_amd import _lib
    res = _lib.BgzfResult()
    assert _lib.lib().sfgpu_bgzf_inflate_host(data, len(data), 1, None, 1 << 40, C.byref(res), None) == OK
    assert (res.n_members, res.consumed, res.n_bytes_out) == (len(payload) // 65280 + 2, len(data), len(payload))


@pytest.mark.gpu
def test_errors_reach_the_caller(gpu, harness):
    from sailfish_amd import _lib
    good = hand_members()["foreign_subfield"][0]
    for name, (member, kind) in error_members().items():
        for data, index in ((member, 0), (good + good + member + good, 2)):
            want = harness.inflate(data)
            got = device_inflate(gpu, data)
            same(got, want, name)
            assert got["rc"] == ERR_FORMAT and got["error"] == (kind, index), (name, got["error"])
        assert b"member 2" in _lib.lib().sfgpu_last_error()
    errs = error_members()
    data = good + errs["crc"][0] + errs["distance_too_far"][0] + errs["no_bc"][0] + good
    same(device_inflate(gpu, data), harness.inflate(data), "several")
    assert device_inflate(gpu, data)["error"] == (CRC_MISMATCH, 1)


@pytest.mark.gpu
def test_error_behind_reused_staging_slots(gpu, harness):
    """300 stored members of 64 KB are 19 MB: the two pinned slots (4 MiB each) are taken again and again; the member behind them
    has a bad CRC; the same file without it inflates whole"""
    from sailfish_amd import gzfile
    noise = np.random.default_rng(45).integers(0, 256, 65280, dtype=np.uint8).tobytes()
    member = gzfile.bgzf_member(noise, 0)
    bad = error_members()["crc"][0]
    data = member * 300 + bad + member
    assert len(data) > 4 * (4 << 20)
    got = device_inflate(gpu, data)
    assert got["rc"] == ERR_FORMAT and got["error"] == (CRC_MISMATCH, 300) and got["n_members"] == 302
    same(got, harness.inflate(data), "300")
    data = member * 300 + gzfile.BGZF_EOF
    got = device_inflate(gpu, data)
    same(got, harness.inflate(data), "300 good")
    assert got["rc"] == OK and got["out"] == noise * 300 and got["blocks"][0] >= 300 and got["blocks"][1:] == (1, 0) and got["error"] == (0, NONE)


# ---- sfgpu_reads_parse_device ----------------------------------------------------------------------------------------------

def both_parses(gpu, text, final, max_reads=1 << 40, cap_bases=1 << 40):
    """(sfgpu_reads_parse_host, sfgpu_reads_parse_device) on the same bytes -> two dicts of every output"""
    import torch
    from sailfish_amd import _lib
    text = bytes(text)
    n = len(text)
    max_reads, cap_bases = min(max_reads, n + 1), min(cap_bases, n)
    outs = []
    for entry in ("host", "device"):
        bases = torch.zeros(max(cap_bases, 16), dtype=torch.uint8, device=gpu)
        off = torch.full((max_reads + 1,), -1, dtype=torch.int64, device=gpu)
        span = torch.zeros(2 * max_reads + 2, dtype=torch.int64, device=gpu)
        res = _lib.ReadsResult()
        with torch.cuda.device(gpu):
            if entry == "host":
                rc = _lib.lib().sfgpu_reads_parse_host(text, n, int(final), max_reads, _lib.ptr(bases), cap_bases, _lib.ptr(off), _lib.ptr(span),
                                                       C.byref(res), _lib.current_stream_ptr())
            else:
                cap_text = ((n + 1 + 15) & ~15) + 16
                d_text = torch.full((cap_text + 16,), 0x41, dtype=torch.uint8, device=gpu)      # 'A' behind the text: the call must pad it
                d_text[:n] = torch.frombuffer(bytearray(text), dtype=torch.uint8).to(gpu) if n else d_text[:0]
                rc = _lib.lib().sfgpu_reads_parse_device(_lib.ptr(d_text), n, cap_text, int(final), max_reads, _lib.ptr(bases), cap_bases,
                                                         _lib.ptr(off), _lib.ptr(span), C.byref(res), _lib.current_stream_ptr())
                assert bytes(d_text[:n].cpu().numpy()) == text and (d_text[cap_text:] == 0x41).all() and res.ms_copy == 0
        d = {k: getattr(res, k) for k, _ in res._fields_ if not k.startswith("ms_")}
        d.update(rc=rc, bases=bases.cpu().numpy().tobytes(), off=off.cpu().numpy().tobytes(),
                 span=span.cpu().numpy()[: 2 * res.n_reads].tobytes())
        outs.append(d)
    return outs


def parses_agree(gpu, text, final, **kw):
    host, dev = both_parses(gpu, text, final, **kw)
    for k in host:
        assert host[k] == dev[k], (k, host[k] if k not in ("bases", "off", "span") else "...", text[:80], final, kw)
    return dev


@pytest.mark.gpu
@pytest.mark.parametrize("shape", sorted(SHAPES))
def test_parse_device_equals_parse_host(gpu, shape):
    rng = np.random.default_rng(sorted(SHAPES).index(shape))
    text, seqs, _ = SHAPES[shape](rng)
    assert len(text) < 65536
    r = parses_agree(gpu, text, 1)
    assert r["rc"] == OK and r["n_reads"] == len(seqs) and r["consumed"] == len(text)
    parses_agree(gpu, text, 0)
    for cut in (len(text) - 1, len(text) // 2, 5):
        for final in (0, 1):
            parses_agree(gpu, text[:cut], final)
    total = sum(len(s) for s in seqs)
    parses_agree(gpu, text, 1, max_reads=3)
    parses_agree(gpu, text, 1, cap_bases=total // 2)


@pytest.mark.gpu
def test_parse_device_large_blank_and_broken(gpu):
    rec, _, _ = fastq_text(np.random.default_rng(6), 1, lens=[1001])
    text = rec * ((8 << 20) // len(rec) + 3)             # three sub-chunks of the host entry
    for final in (0, 1):
        r = parses_agree(gpu, text, final)
        assert r["rc"] == OK and r["n_reads"] == len(text) // len(rec)
    lines = text.split(b"\n")
    lines[-3] = b""
    assert parses_agree(gpu, b"\n".join(lines), 1)["rc"] == ERR_FORMAT
    for blank in (b"\n", b"\r\n\n\n", b"\n" * 70000, b"\n\nx\n"):
        for final in (0, 1):
            parses_agree(gpu, blank, final)
    parses_agree(gpu, b"", 1)
    from sailfish_amd import _lib
    import torch
    t = torch.zeros(64, dtype=torch.uint8, device=gpu)
    res = _lib.ReadsResult()
    assert _lib.lib().sfgpu_reads_parse_device(_lib.ptr(t), 20, 32, 1, 1, _lib.ptr(t), 0, _lib.ptr(t), None, C.byref(res), None) == 1     # cap_text


# ---- ReadFile ----------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def text_files(tmp_path_factory):
    from sailfish_amd import gzfile
    d = tmp_path_factory.mktemp("bgzf_files")
    text = text_3000()
    (d / "reads.fastq").write_bytes(text)
    gzfile.write_bgzf(d / "reads.fastq.bgz", text)
    with gzip.open(d / "reads.fastq.gz", "wb", compresslevel=6) as f:
        f.write(text)
    return d, text


def read_all(path, gpu, batch, **kw):
    from sailfish_amd import readfile
    got_b, got_o, names = [], [np.zeros(1, np.int64)], []
    with readfile.ReadFile(path, gpu, names=True, **kw) as rf:
        while True:
            b, o = rf.read(batch)
            n = o.numel() - 1
            if n == 0:
                break
            o = o.cpu().numpy()
            got_b.append(b.cpu().numpy()[: o[-1]]); got_o.append(o[1:] + got_o[-1][-1]); names += rf.last_names
        return np.concatenate(got_b), np.concatenate(got_o), names, rf.inflate, dict(rf.stats)


@pytest.fixture(scope="module")
def plain_result(gpu, text_files):
    d, _ = text_files
    return read_all(d / "reads.fastq", gpu, 1 << 40)


@pytest.mark.gpu
@pytest.mark.parametrize("block_bytes", [20_000, 100_000, 32 << 20])
@pytest.mark.parametrize("batch", [1, 7, 1000, 1 << 40])
def test_read_file_bgzf_equals_plain(gpu, text_files, plain_result, block_bytes, batch):
    d, text = text_files
    b, o, names, inflate, stats = read_all(d / "reads.fastq.bgz", gpu, batch, block_bytes=block_bytes)
    assert inflate == "device" and plain_result[3] is None
    assert np.array_equal(b, plain_result[0]) and np.array_equal(o, plain_result[1]) and names == plain_result[2]
    assert stats["members"] == -(-len(text) // 65280) + 1 and stats["bytes_compressed"] == os.path.getsize(d / "reads.fastq.bgz")
    assert stats["ms_inflate"] > 0


@pytest.mark.gpu
def test_read_file_host_paths_and_errors(gpu, text_files, plain_result, tmp_path):
    from sailfish_amd import gzfile, readfile
    d, text = text_files
    for path, kw in ((d / "reads.fastq.gz", {}), (d / "reads.fastq.bgz", dict(inflate="host"))):
        b, o, names, inflate, stats = read_all(path, gpu, 1000, **kw)
        assert inflate == "host" and stats["members"] == 0
        assert np.array_equal(b, plain_result[0]) and np.array_equal(o, plain_result[1]) and names == plain_result[2]
    # a malformed record behind a member boundary: the record number counts from the start of the file
    lines = text.split(b"\n")
    rec = 2000
    assert len(b"\n".join(lines[: 4 * rec])) > 5 * 65280
    lines[4 * rec + 2] = b"-"
    gzfile.write_bgzf(tmp_path / "bad_record.bgz", b"\n".join(lines))
    with readfile.ReadFile(tmp_path / "bad_record.bgz", gpu, block_bytes=50_000) as rf:
        assert rf.inflate == "device"
        with pytest.raises(ValueError, match=r"bad_record\.bgz: record 2000 .*'\+'"):
            for _ in range(10):
                rf.read(500)
    # a corrupt member: its number and where it begins
    data = bytearray((d / "reads.fastq.bgz").read_bytes())
    p = 0
    for _ in range(4):
        p += int.from_bytes(data[p + 16:p + 18], "little") + 1
    end = p + int.from_bytes(data[p + 16:p + 18], "little") + 1
    data[end - 8] ^= 1                                    # the CRC of member 4
    (tmp_path / "bad_member.bgz").write_bytes(data)
    for block in (30_000, 32 << 20):
        with readfile.ReadFile(tmp_path / "bad_member.bgz", gpu, block_bytes=block) as rf:
            with pytest.raises(ValueError, match=rf"bad_member\.bgz: gzip member 4 \(byte {p} of the file\).*CRC"):
                rf.read(1 << 40)
    (tmp_path / "cut.bgz").write_bytes(bytes(data[: end - 3]))
    with readfile.ReadFile(tmp_path / "cut.bgz", gpu) as rf:
        with pytest.raises(ValueError, match=r"gzip member 4 \(byte %d of the file\).*ends before" % p):
            rf.read(1 << 40)


@pytest.mark.gpu
def test_quantify_files_from_bgzf_writes_the_same_quant_sf(gpu, tmp_path):
    import sailfish_amd as sf
    from sailfish_amd import gzfile
    names, seqs, r1, r2 = _sample()
    plain = _render(tmp_path, names, seqs, r1, r2)
    opts = dict(batch_reads=3000, cmd_options={"libType": "IU"}, device=gpu)
    rc, exp = sf.mapper.quantify_files(*plain, "IU", str(tmp_path / "plain"), sf.SailfishOpts(numFragSamples=5000), **opts)
    assert rc == 0 and exp.numMappedFragments() == 10000
    blocked = []
    for p in plain:
        blocked.append(str(p) + ".bgz")
        gzfile.write_bgzf(blocked[-1], p.read_bytes())
        assert gzip.decompress(open(blocked[-1], "rb").read()) == p.read_bytes()
    rc, exp = sf.mapper.quantify_files(*blocked, "IU", str(tmp_path / "bgzf"), sf.SailfishOpts(numFragSamples=5000), **opts)
    assert rc == 0 and exp.numMappedFragments() == 10000
    assert (tmp_path / "bgzf" / "quant.sf").read_bytes() == (tmp_path / "plain" / "quant.sf").read_bytes()
