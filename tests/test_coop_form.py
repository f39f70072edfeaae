"""CPU pin of the cooperative kernels' form selector (csrc/rle_coop_limits.h coop_enc_form /
coop_dec_form): which template instantiation of csrc/rle_coop.hip sizes select.
tests/native/coop_form_check.cpp includes only that header, is built with plain g++ and prints the
form of each query; the expected rows below are written out by hand from the if-chains the four
launchers carried before the selector had a home of its own, one row on each side of every
threshold.  The library's host-only query (rle_mi355x_coop_form) must agree, and the set of forms
the selector can return must be exactly the forms rle_coop.hip instantiates, batched and by value.
"""
import os
import re
import shutil
import subprocess

import pytest

import rle_mi355x as R

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "c-filestorage-server-and-client_amd", "csrc")
SRC = os.path.join(REPO, "tests", "native", "coop_form_check.cpp")

pytestmark = pytest.mark.skipif(shutil.which("g++") is None, reason="needs g++")

ENC_FORMS = [(2, 1), (3, 1), (4, 1), (6, 1), (8, 1), (12, 1), (16, 1), (16, 2), (16, 4)]
DEC_FORMS = [(2, 4096, 1), (3, 4096, 1), (5, 4096, 1), (8, 4096, 1),
             (2, 16384, 1), (3, 16384, 1), (5, 16384, 1), (8, 16384, 1), (12, 16384, 1), (16, 16384, 1),
             (16, 16384, 2),
             (4, 32768, 1), (8, 32768, 1), (16, 32768, 1), (16, 32768, 3), (16, 32768, 4),
             (16, 65536, 5)]

# (max_len, form)
ENC = [
    (0, None), (1, None), (1024, None),
    (1025, (2, 1)), (2048, (2, 1)),
    (2049, (3, 1)), (3072, (3, 1)),
    (3073, (4, 1)), (4096, (4, 1)),
    (4097, (6, 1)), (6144, (6, 1)),
    (6145, (8, 1)), (8192, (8, 1)),
    (8193, (12, 1)), (12288, (12, 1)),
    (12289, (16, 1)), (16384, (16, 1)),
    (16385, (16, 2)), (32768, (16, 2)),
    (32769, (16, 4)), (65536, (16, 4)),
    (65537, None), (1 << 32, None), ((1 << 32) + 2048, None),
]

# (max_in_len, max_out_len, form)
DEC = [
    # the stream length limits, in every band
    (1008, 1, None), (1008, 4096, None), (1008, 16384, None), (1008, 32768, None), (1008, 65536, None),
    (1009, 0, (2, 4096, 1)), (1009, 4096, (2, 4096, 1)), (1009, 4097, (2, 16384, 1)), (1009, 16384, (2, 16384, 1)),
    (1009, 16385, (4, 32768, 1)), (1009, 32768, (4, 32768, 1)), (1009, 32769, (16, 65536, 5)),
    (1009, 65536, (16, 65536, 5)), (1009, 65537, None),
    (80640, 1, (16, 16384, 2)), (80640, 4096, (16, 16384, 2)), (80640, 16384, (16, 16384, 2)),
    (80640, 16385, (16, 32768, 4)), (80640, 32768, (16, 32768, 4)), (80640, 32769, (16, 65536, 5)),
    (80640, 65536, (16, 65536, 5)), (80640, 65537, None),
    (80641, 1, None), (80641, 4096, None), (80641, 16384, None), (80641, 32768, None), (80641, 65536, None),
    ((1 << 32) + 2016, 4096, None), (2016, (1 << 32) + 4096, None),
    # out <= 4096
    (2016, 4096, (2, 4096, 1)), (2017, 4096, (3, 4096, 1)), (3024, 4096, (3, 4096, 1)),
    (3025, 4096, (5, 4096, 1)), (5040, 4096, (5, 4096, 1)), (5041, 4096, (8, 4096, 1)),
    (8064, 4096, (8, 4096, 1)), (8065, 4096, (8, 4096, 1)), (16128, 4096, (8, 4096, 1)),
    # past 16 tiles the two-round form, before the 4096 band is looked at
    (16129, 4096, (16, 16384, 2)), (16129, 1, (16, 16384, 2)), (32256, 4096, (16, 16384, 2)),
    (32257, 4096, (16, 16384, 2)),
    # 4096 < out <= 16384
    (2016, 4097, (2, 16384, 1)), (2017, 4097, (3, 16384, 1)),
    (2016, 16384, (2, 16384, 1)), (2017, 16384, (3, 16384, 1)), (3024, 16384, (3, 16384, 1)),
    (3025, 16384, (5, 16384, 1)), (5040, 16384, (5, 16384, 1)), (5041, 16384, (8, 16384, 1)),
    (8064, 16384, (8, 16384, 1)), (8065, 16384, (12, 16384, 1)), (12096, 16384, (12, 16384, 1)),
    (12097, 16384, (16, 16384, 1)), (16128, 16384, (16, 16384, 1)), (16129, 16384, (16, 16384, 2)),
    (32256, 16384, (16, 16384, 2)), (32257, 16384, (16, 16384, 2)),
    # 16384 < out <= 32768
    (4032, 16385, (4, 32768, 1)), (4033, 16385, (8, 32768, 1)),
    (4032, 32768, (4, 32768, 1)), (4033, 32768, (8, 32768, 1)), (8064, 32768, (8, 32768, 1)),
    (8065, 32768, (16, 32768, 1)), (16128, 32768, (16, 32768, 1)), (16129, 32768, (16, 32768, 3)),
    (32256, 32768, (16, 32768, 3)), (32257, 32768, (16, 32768, 3)),
    (48384, 32768, (16, 32768, 3)), (48385, 32768, (16, 32768, 4)), (48384, 16385, (16, 32768, 3)),
    (48385, 16385, (16, 32768, 4)), (64512, 32768, (16, 32768, 4)), (64513, 32768, (16, 32768, 4)),
    # 32768 < out <= 65536: one form
    (2016, 32769, (16, 65536, 5)), (16128, 65536, (16, 65536, 5)), (16129, 65536, (16, 65536, 5)),
    (48385, 65536, (16, 65536, 5)), (64512, 65536, (16, 65536, 5)), (64513, 32769, (16, 65536, 5)),
]


@pytest.fixture(scope="module")
def form_check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("coop_form") / "coop_form_check")
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-Werror", "-I" + CSRC, SRC, "-o", exe], check=True)

    def ask(queries):
        r = subprocess.run([exe], input="\n".join(queries) + "\n", capture_output=True, text=True, timeout=120)
        assert r.returncode == 0, (r.returncode, r.stderr)
        return r.stdout.splitlines()

    return ask


def _form(line):
    return None if line == "none" else tuple(int(x) for x in line.split())


def test_encode_rows(form_check):
    got = form_check([f"enc {u}" for u, _ in ENC])
    assert len(got) == len(ENC)
    for (u, want), g in zip(ENC, got):
        assert _form(g) == want, (u, g)
        assert R.coop_enc_form(u) == want, u


def test_decode_rows(form_check):
    got = form_check([f"dec {c} {u}" for c, u, _ in DEC])
    assert len(got) == len(DEC)
    for (c, u, want), g in zip(DEC, got):
        assert _form(g) == want, (c, u, g)
        assert R.coop_dec_form(c, u) == want, (c, u)


def test_rows_name_every_form():
    assert {f for _, f in ENC if f} == set(ENC_FORMS) and len(ENC_FORMS) == 9
    assert {f for _, _, f in DEC if f} == set(DEC_FORMS) and len(DEC_FORMS) == 17


def test_selector_returns_exactly_the_forms(form_check):
    """Over every input length (decode: every stream length against the output lengths at and
    around every multiple of 4096 and a ladder between) the selector returns the 9 + 17 forms and no
    other."""
    got = form_check(["all"])
    enc = {tuple(int(x) for x in g.split()[1:]) for g in got if g.startswith("enc")}
    dec = {tuple(int(x) for x in g.split()[1:]) for g in got if g.startswith("dec")}
    assert enc == set(ENC_FORMS) and dec == set(DEC_FORMS), (enc, dec)


def test_launchers_instantiate_exactly_the_forms():
    """rle_coop.hip lists the forms once per direction (RLE_COOP_ENC_FORMS / RLE_COOP_DEC_FORMS); the
    batched and the by-value launcher of each direction expand that list into their kernels'
    instantiations, and nothing else in the file launches a cooperative codec kernel."""
    src = open(os.path.join(CSRC, "rle_coop.hip")).read()
    src = re.sub(r"\\\n", " ", src)

    def listed(name):
        m = re.search(r"#define %s\(X\)([^\n]*)" % name, src)
        assert m, name
        return [tuple(int(x) for x in t.split(",")) for t in re.findall(r"X\(([^)]*)\)", m.group(1))]

    assert sorted(listed("RLE_COOP_ENC_FORMS")) == sorted(ENC_FORMS)
    assert sorted(listed("RLE_COOP_DEC_FORMS")) == sorted(DEC_FORMS)
    for kernel, forms, macro in (("enc_coop_kernel", "RLE_COOP_ENC_FORMS", "RLE_ENC_COOP"),
                                 ("enc_coop_one_kernel", "RLE_COOP_ENC_FORMS", "RLE_ENC_ONE"),
                                 ("dec_coop_kernel", "RLE_COOP_DEC_FORMS", "RLE_DEC_COOP"),
                                 ("dec_coop_one_kernel", "RLE_COOP_DEC_FORMS", "RLE_DEC_ONE")):
        launches = re.findall(r"hipLaunchKernelGGL\(\(rle::%s<([^>]*)>\)" % kernel, src)
        assert len(launches) == 1 and "_" in launches[0], (kernel, launches)   # the macro's own parameters
        assert len(re.findall(r"%s\(%s\)" % (forms, macro), src)) == 1, (kernel, macro)
    assert "coop_enc_form(max_len)" in src and "coop_enc_form(U)" in src
    assert "coop_dec_form(max_in_len, max_out_len)" in src and "coop_dec_form(C, U)" in src
