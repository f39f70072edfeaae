"""CPU test of the drop-in's call routing (csrc/rle_route.h): which path a call of given sizes takes
under given settings.  tests/native/route_check.cpp includes only that header, is built with plain
g++ and prints the route of each query; the expected routes below are written out by hand from the
expressions the drop-in used before the routing had a file of its own, one row per threshold edge.

In the rows, `reg` is "registration wanted" (before reg_likely), a body other than "large" is a small
body, and "mapped_seg" is the segmented kernels on the mapped buffer.
"""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "c-filestorage-server-and-client_amd", "csrc")
SRC = os.path.join(REPO, "tests", "native", "route_check.cpp")

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")

# (settings, call, reg, body)
CALLS = [
    ("", "compress 49151", 0, "mapped_one"),
    ("", "compress 49152", 0, "mapped_one"),
    ("", "compress 65536", 0, "mapped_one"),
    ("", "compress 65537", 0, "mapped_seg"),
    ("", "compress 262144", 0, "mapped_seg"),
    ("", "compress 262145", 1, "large"),
    ("", "decompress 32767 131072 0", 0, "mapped_one"),
    ("", "decompress 32767 131072 1", 0, "mapped_one"),
    ("", "decompress 32768 65536 0", 0, "mapped_one"),
    ("", "decompress 32768 65537 0", 0, "mapped_seg"),
    ("", "decompress 80640 65536 4096", 0, "mapped_one"),
    ("", "decompress 80641 65536 0", 0, "mapped_seg"),
    # at U + E = 393216 a decompress both wants registration and is within the mapped
    # buffer's reach.  These two rows record the present behaviour, which the fix will change on purpose.
    ("", "decompress 100000 262143 131073", 1, "mapped_seg"),
    ("", "decompress 100000 262145 131071", 1, "mapped_seg"),
    ("", "decompress 100000 262145 131072", 1, "large"),
    ("", "decompress 1000 65537 200000", 1, "mapped_one"),
    ("", "decompress 262145 300000 0", 1, "large"),
    ("zc_coop=0", "compress 49151", 0, "mapped_seg"),
    ("zc_coop=0", "compress 49152", 0, "mapped_seg"),
    ("zc_coop=0", "compress 65536", 0, "mapped_seg"),
    ("zc_coop=0", "decompress 32768 65536 0", 0, "mapped_seg"),
    ("zc_seg=0", "compress 49151", 0, "mapped_one"),
    ("zc_seg=0", "compress 49152", 0, "large"),
    ("zc_seg=0", "decompress 32767 131072 0", 0, "mapped_one"),
    ("zc_seg=0", "decompress 32767 131072 1", 0, "large"),
    ("zerocopy=0", "compress 49151", 0, "staged"),
    ("zerocopy=0", "compress 49152", 0, "large"),
    ("zerocopy=0", "decompress 32767 131072 0", 0, "staged"),
    ("zerocopy=0", "decompress 32767 131072 1", 0, "large"),
    ("reg_min=0", "compress 262145", 0, "large"),
    ("reg_min=0", "decompress 100000 262145 131071", 0, "mapped_seg"),
    ("fake_devs=2", "compress 262145", 0, "large"),
]

# the kernels of a buffer in device memory: (call, segmented, output travels with its size)
DEVICE_FORMS = [
    ("compress 49151", 0, 1),
    ("compress 49152", 1, 1),
    ("compress 131072", 1, 1),
    ("compress 131073", 1, 0),
    ("decompress 32767 40000 0", 0, 0),
    ("decompress 32768 40000 0", 1, 0),
]

# (settings, C, U, A, route)
APPENDS = [
    ("", 4096, 4096, 4096, "mapped"),
    ("", 4096, 61440, 4096, "mapped"),
    ("", 4096, 61441, 4096, "small_splice"),
    ("", 40000, 65536, 0, "mapped"),
    ("", 40000, 65537, 0, "large_splice"),
    ("", 1000, 200000, 1000, "small_splice"),
    ("", 1000, 200000, 49136, "large_splice"),
    ("", 0, 100, 100, "large_splice"),
    ("zc_coop=0", 4096, 61440, 4096, "small_splice"),
    ("zc_coop=0", 40000, 65536, 0, "large_splice"),
    ("zc_coop=0", 4096, 4096, 4096, "mapped"),
    # nothing is mapped without zero-copy: what the splice conditions alone decide
    ("zerocopy=0", 4096, 4096, 4096, "small_splice"),
    ("zerocopy=0", 4096, 61440, 4096, "small_splice"),
    ("zerocopy=0", 40000, 65536, 0, "large_splice"),
    # the shapes tests/test_gpu_append_splice.py relies on to reach each splice route (the smallest and
    # largest C, U and A of each of its batteries).  Behind the 66 000-byte run carrier (C about 22 KB):
    ("", 22005, 66003, 0, "small_splice"),
    ("", 22005, 66003, 50, "small_splice"),
    ("", 22010, 66010, 0, "small_splice"),
    ("", 22010, 66010, 50, "small_splice"),
    ("", 22226, 66437, 103, "small_splice"),
    ("", 22106, 66204, 218, "small_splice"),
    ("", 23369, 70092, 21, "small_splice"),
    ("", 26102, 78289, 21, "small_splice"),
    ("", 22005, 66003, 49135, "small_splice"),
    ("", 22005, 66003, 49136, "large_splice"),
    ("", 22007, 66011, 140000, "large_splice"),
    # behind the literal carrier (C past 64 KiB)
    ("", 66267, 66003, 0, "large_splice"),
    ("", 66100, 66010, 0, "large_splice"),
    ("", 66100, 66010, 50, "large_splice"),
    ("", 66488, 66437, 103, "large_splice"),
    ("", 70364, 78289, 21, "large_splice"),
    ("", 66267, 66003, 49135, "large_splice"),
    ("", 66269, 66011, 140000, "large_splice"),
    # a file that is one run
    ("", 22002, 66000, 0, "small_splice"),
    ("", 22005, 66008, 3, "small_splice"),
    ("", 33334, 100000, 0, "large_splice"),
    ("", 33336, 100008, 3, "large_splice"),
    # streams that are not encoder output (U short of and past the decoded length, no stream) and the
    # call that fills the decode buffer before each
    ("", 23334, 70000, 0, "small_splice"),
    ("", 22010, 66048, 40, "small_splice"),
    ("", 22009, 66010, 0, "small_splice"),
    ("", 66272, 66048, 40, "large_splice"),
    ("", 66271, 66010, 0, "large_splice"),
    ("", 0, 70000, 40, "large_splice"),
    # the tiny streams with the zero-copy form off
    ("zerocopy=0", 1, 1, 0, "small_splice"),
    ("zerocopy=0", 1, 1, 133, "small_splice"),
    ("zerocopy=0", 3, 1, 1, "small_splice"),
    ("zerocopy=0", 222, 435, 103, "small_splice"),
    ("zerocopy=0", 102, 202, 218, "small_splice"),
]

# (settings, C, U, route)
READN = [
    ("", 32767, 16384, "mapped"),
    ("", 32767, 16385, "staged"),
    ("", 32768, 16384, "staged_seg"),
    ("zerocopy=0", 32767, 16384, "staged"),
    ("zerocopy=0", 32768, 16384, "staged_seg"),
]


@pytest.fixture(scope="module")
def route_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("route") / "route_check")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Werror", "-I" + CSRC, SRC, "-o", exe], check=True)

    def ask(queries):
        r = subprocess.run([exe], input="\n".join(queries) + "\n", capture_output=True, text=True, timeout=60)
        assert r.returncode == 0, (r.returncode, r.stderr)
        out = r.stdout.splitlines()
        assert len(out) == len(queries)
        return [dict(kv.split("=") for kv in line.split()) for line in out]

    return ask


def test_compress_and_decompress_routes(route_check):
    got = route_check([f"{s} {call}" for s, call, _, _ in CALLS])
    for (s, call, reg, body), g in zip(CALLS, got):
        assert (int(g["reg"]), g["body"]) == (reg, body), (s, call, g)


def test_device_forms(route_check):
    got = route_check([call for call, _, _ in DEVICE_FORMS])
    for (call, seg, one_trip), g in zip(DEVICE_FORMS, got):
        assert (int(g["dev_seg"]), int(g["one_trip"])) == (seg, one_trip), (call, g)


def test_append_routes(route_check):
    """The worst-case compressed sizes the append route compares come from the library's own
    rle_max_compressed_size, as in the drop-in."""
    import rle_mi355x as R
    got = route_check([f"{s} append {C} {U} {A} {R.max_compressed_size(U + A)} {R.max_compressed_size(16 + A)}"
                       for s, C, U, A, _ in APPENDS])
    for row, g in zip(APPENDS, got):
        assert g["append"] == row[4], (row, g)


def test_readn_file_routes(route_check):
    got = route_check([f"{s} readn {C} {U}" for s, C, U, _ in READN])
    for row, g in zip(READN, got):
        assert g["readn"] == row[3], (row, g)
