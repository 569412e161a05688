"""The aliasing contract checked on the CPU: the table of tests/test_gpu_aliasing.py against the prototypes and the comments of
include/scl_hip.h, and the span helper (include/scl_hip/detail/span.hpp) through its stand-alone host program.

* every entry point that is a row of test_gpu_redzones.TABLE (the ones that write device memory through a caller's pointer; its
  EXEMPT ones are left out) has a decision -- permit or refuse -- for every (non-const *_dev parameter, other *_dev parameter) pair
  of its prototype, and for no other pair: adding an entry point, or a device operand to one, without deciding fails here;
* the words of each decision stand in the comment right in front of that prototype, so the header and the tests cannot drift;
* the aliases that must stay permitted (the header's and the reference's *InPlace members) are permitted;
* tests/cxx/span_overlap_check.cc passes plain and under -fsanitize=address,undefined as a host binary.
"""
import os
import re
import subprocess

import pytest

from abi_support import ENGINE, declared_symbols

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CXX = os.path.join(ROOT, "tests", "cxx")


def header():
    return open(os.path.join(ROOT, "include", "scl_hip.h")).read()


def prototypes():
    """{entry point: (its parameter list [(type, name)], the comments between the previous declaration and it)}"""
    src = header()
    out, prev = {}, 0
    for m in re.finditer(r"^(?:int|size_t|const char\*) (scl_hip_\w+)\s*\(([^;]*?)\)\s*;", src, flags=re.M | re.S):
        between = src[prev:m.start()]          # from the previous prototype; a #define or a typedef in between starts afresh
        prev = m.end()
        for stop in ("#define", "typedef", 'extern "C" {'):
            between = between[between.rfind(stop) + 1:] if stop in between else between
        comment = " ".join(re.findall(r"/\*(.*?)\*/", between, flags=re.S))
        comment = re.sub(r"\s+", " ", re.sub(r"^\s*\*", " ", comment, flags=re.M))
        params = []
        for p in re.sub(r"\s+", " ", m.group(2)).split(","):
            p = p.strip()
            if p in ("void", ""):
                continue
            pm = re.match(r"(.*?)(\w+)(\[\d*\])?$", p)
            params.append(((pm.group(1) + (pm.group(3) or "")).strip(), pm.group(2)))
        out[m.group(1)] = (params, comment)
    return out


def device_operands(params):
    """(written, all): the *_dev pointer parameters that are not const, and all *_dev pointer parameters"""
    dev = [(t, n) for t, n in params if n.endswith("_dev") and "*" in t]
    return [n for t, n in dev if "const" not in t], [n for t, n in dev]


def test_the_parser_reads_the_header_as_test_abi_does():
    protos = prototypes()
    assert sorted(protos) == declared_symbols(ENGINE)
    params, comment = protos["scl_hip_ec_mul"]
    assert [n for _, n in params] == ["dst_dev", "points_dev", "scalars_dev", "scratch_dev", "n", "stream"]
    assert device_operands(params) == (["dst_dev", "scratch_dev"], ["dst_dev", "points_dev", "scalars_dev", "scratch_dev"])
    assert "Aliasing:" in comment and "scl_hip_ec_mul_scratch_bytes" not in comment.split("Aliasing:")[1]


def test_every_writing_entry_point_has_a_decision_for_every_pair_of_device_operands():
    import test_gpu_aliasing as T
    import test_gpu_redzones as G
    protos = prototypes()
    assert set(T.ALIASING) == set(G.TABLE), sorted(set(T.ALIASING) ^ set(G.TABLE))
    assert not set(T.ALIASING) & set(G.EXEMPT)
    for entry, pairs in T.ALIASING.items():
        written, every = device_operands(protos[entry][0])
        assert written, f"{entry} writes no device operand and is a row of the red-zone table?"
        want = {(o, x) for o in written for x in every if x != o}
        assert set(pairs) == want, f"{entry}: undecided {sorted(want - set(pairs))}, not in the prototype {sorted(set(pairs) - want)}"
        for (o, x), (kind, words) in pairs.items():
            assert kind in ("permit", "refuse"), (entry, o, x)
            assert isinstance(words, str) and (o in words or x in words), (entry, o, x, words)
        assert (entry in T.SOLE) == (len(every) == 1), entry


def test_each_decision_is_worded_in_the_comment_of_its_entry_point():
    import test_gpu_aliasing as T
    protos = prototypes()
    for entry, pairs in T.ALIASING.items():
        comment = protos[entry][1]
        assert "Aliasing:" in comment, f"{entry}: no aliasing rule in front of its prototype"
        rule = comment.split("Aliasing:")[-1]
        for (o, x), (kind, words) in pairs.items():
            assert words in rule, f"{entry}: ({o}, {x}) is decided as {words!r}; the header says {rule.strip()!r}"
        if entry in T.SOLE:
            assert T.SOLE[entry] in rule, entry
        # and the header permits nothing the table refuses
        for o, x in re.findall(r"(\w+_dev) may be (\w+_dev)", rule):
            written, _ = device_operands(protos[entry][0])
            if o in written:
                assert pairs[(o, x)][0] == "permit", f"{entry}: the header permits {o} on {x}, the table refuses it"


def test_the_conventions_state_the_rule():
    conv = re.sub(r"\s+", " ", re.sub(r"^\s*\*", " ", header().split("#ifndef SCL_HIP_H")[0], flags=re.M))
    for words in ("an output may COINCIDE with an input only where the entry point says so", "the same pointer and, for matrices, the same stride",
                  "SCL_ERR_BAD_ARG", "names both operands", "before anything is launched or written",
                  "[ptr, ptr + ((rows - 1) * stride + cols) * element bytes)", "Empty operands"):
        assert words in conv, words


MUST_STAY = [("scl_hip_ew", "dst_dev", "a_dev"), ("scl_hip_ew", "dst_dev", "b_dev"), ("scl_hip_ew_status", "dst_dev", "a_dev"),
             ("scl_hip_ew_status", "dst_dev", "b_dev"), ("scl_hip_scalar_mul", "dst_dev", "a_dev"), ("scl_hip_ec_ew", "dst_dev", "a_dev"),
             ("scl_hip_ec_ew", "dst_dev", "b_dev"), ("scl_hip_ec_mul", "dst_dev", "points_dev"),
             ("scl_hip_merkle_build", "tree_dev", "leaf_digests_dev")]


def test_the_promised_aliases_stay_permitted_and_the_named_ones_are_refused():
    import test_gpu_aliasing as T
    for entry, o, x in MUST_STAY:
        assert T.ALIASING[entry][(o, x)][0] == "permit", (entry, o, x)
    for entry, o, x in [("scl_hip_matmul", "C_dev", "A_dev"), ("scl_hip_matmul", "C_dev", "B_dev"), ("scl_hip_ec_lincomb", "dst_dev", "points_dev"),
                        ("scl_hip_ec_matmul", "dst_dev", "points_dev")]:
        assert T.ALIASING[entry][(o, x)][0] == "refuse", (entry, o, x)
    for entry in ("scl_hip_feldman_verify", "scl_hip_pedersen_verify", "scl_hip_ec_mul", "scl_hip_ecdsa_verify"):
        scratch = [o for (o, _) in T.ALIASING[entry] if o.startswith("scratch")]
        assert scratch and all(kind == "refuse" for (o, x), (kind, _) in T.ALIASING[entry].items() if o in scratch or x in scratch), entry


def test_every_refusal_case_has_a_placement_and_every_pair_a_case():
    """the refusal cases of test_gpu_aliasing are built from the table: every pair is there for every field of its entry point"""
    import test_gpu_aliasing as T
    seen = {(e, o, x) for e, o, x, f, kind in T.REFUSALS}
    assert seen == {(e, o, x) for e, pairs in T.ALIASING.items() for (o, x) in pairs}
    ids = [(e, o, x, f) for e, o, x, f, kind in T.REFUSALS]
    assert len(ids) == len(set(ids))


def span_check(tmp_path, name, flags):
    exe = str(tmp_path / name)
    b = subprocess.run(["g++", "-std=c++20", "-Wall", "-Wextra", f"-I{ROOT}/include", *flags, "-o", exe, os.path.join(CXX, "span_overlap_check.cc")],
                       capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and " 0 mismatches" in r.stdout, r.stdout + r.stderr
    return r.stdout + r.stderr


def test_the_span_helper_on_touching_overlapping_empty_pitched_and_wrapping_spans(tmp_path):
    span_check(tmp_path, "span_overlap_check", ["-O2"])


def test_the_span_helper_under_the_sanitizers(tmp_path):
    """the same stand-alone host program under -fsanitize=address,undefined: no overflow it does not mean"""
    out = span_check(tmp_path, "span_overlap_check_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"])
    assert "runtime error" not in out and "AddressSanitizer" not in out
