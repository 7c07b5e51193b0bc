"""Writes deflate_writer_digests.json: sha256 and length of the serial gzip stream (tests/gzwrite_harness.cpp over csrc/gzfmt.h) and
of the serial BGZF file (tests/bgzw_harness.cpp over csrc/bgzwfmt.h) for every input set of tests/test_gzwrite_cpu.py and
tests/test_bgzw_cpu.py, with their write cuts; the payloads' own digests go along, so that a changed input is told from a changed
encoder.  The two tests recompute the digests; the GPU suites compare the device bytes with the same serial encoders.

Run it only on purpose, from a commit whose encoders are the ones to pin (the file names that commit): a change that is meant to
keep the bytes must not regenerate it.
    python tests/golden/make_deflate_writer_digests.py
"""
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import __graft_entry__  # noqa: E402
import test_bgzw_cpu as B  # noqa: E402
import test_gzwrite_cpu as G  # noqa: E402


def main():
    if not os.path.exists(os.path.join(ROOT, "oracle", "liboracle.so")):
        __graft_entry__.build()                           # the gzip sets hold the oracle's samples
    commit = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "HEAD"], text=True).strip()
    with tempfile.TemporaryDirectory() as tmp:
        gz = G.build_harness(tmp)
        bgzw = B.Harness(B.build_harness(tmp))
        out = {"encoders_of_commit": commit,
               "gzip": G.stream_digests(lambda data, writes: G.host_encode(gz, tmp, data, writes)[0], G.digest_sets()),
               "bgzf": G.stream_digests(lambda data, writes: bgzw.encode(data, writes)[0], B.digest_sets(bgzw.P))}
    with open(G.DIGESTS, "w") as f:
        json.dump(out, f, indent=0, sort_keys=True)
        f.write("\n")
    print(f"{len(out['gzip'])} gzip streams, {len(out['bgzf'])} BGZF files, encoders of {commit}")


if __name__ == "__main__":
    main()
