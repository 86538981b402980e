"""Expansion factors other than 4, the parts that need no GPU, against the reference's own runs (tests/golden/expansion.json,
make_golden.py --expansion): Fri.num_rounds where the expansion factor stops the halving and where 4 s does, the library's
host-side Fiat-Shamir pieces on the roots of the reference's proofs, its index sampling with the (N/2, last length, s) of those
proofs, and the instances of tests/expansion_cases.py against the recorded shapes."""
import ctypes
import hashlib

from conftest import load_golden
import expansion_cases
import synth
from algebra import Field, FieldElement
from fri import Fri
from ip import ProofStream

field = Field.main()
G = load_golden("expansion.json")


def test_the_records_are_at_other_expansion_factors_and_cover_both_stopping_rules():
    assert all(ef != 4 for _, ef, _, _ in G["num_rounds"])
    assert {ef for _, ef, _, _ in G["num_rounds"]} >= {2, 8, 16, 32, 64}
    stopped_by_ef = [(n, ef, s) for n, ef, s, rounds in G["num_rounds"] if n >> rounds <= ef and n >> rounds > 4 * s]
    stopped_by_4s = [(n, ef, s) for n, ef, s, rounds in G["num_rounds"] if n >> rounds <= 4 * s and n >> rounds > ef]
    assert len(stopped_by_ef) >= 3 and len(stopped_by_4s) >= 3
    assert all(r["expansion_factor"] != 4 for r in G["fri"] + G["stark"])
    assert all(isinstance(r["reference_seconds"], dict) for r in G["fri"] + G["stark"])
    # per shape an honest codeword, which the reference accepts, and one of N / ef + 1 coefficients, which it rejects
    for rec in G["fri"]:
        assert rec["num_coeffs"] == (1 << rec["logN"]) // rec["expansion_factor"] + (0 if rec["honest"] else 1)
        assert rec["verifies"] in (rec["honest"], None)
        assert rec["last_codeword_len"] == (1 << rec["logN"]) >> (rec["num_rounds"] - 1)
    assert sum(r["verifies"] is None for r in G["fri"]) == 2              # (the shape whose last codeword the reference cannot interpolate)


def test_num_rounds():
    for n, ef, s, rounds in G["num_rounds"]:
        assert Fri(field.generator(), field.primitive_nth_root(n), n, ef, s).num_rounds() == rounds, (n, ef, s)
    for rec in G["fri"]:
        n = 1 << rec["logN"]
        fr = Fri(field.generator(), field.primitive_nth_root(n), n, rec["expansion_factor"], rec["num_colinearity_tests"])
        assert fr.num_rounds() == rec["num_rounds"] == len(rec["roots"])


def test_library_fiat_shamir_pieces_on_the_new_roots():
    """as tests/test_host_cpu.py does for fri.json's prove_synth: transcript bytes, SHAKE-256 and sc_field_sample, round by round"""
    import starkcore
    lib = starkcore.lib()

    def c_transcript(items):
        lens = (ctypes.c_uint32 * max(1, len(items)))(*[len(i) for i in items])
        need = ctypes.c_uint64(0)
        assert lib.sc_transcript_bytes(b"".join(items), lens, len(items), None, 0, ctypes.byref(need)) == 0
        buf = ctypes.create_string_buffer(need.value)
        assert lib.sc_transcript_bytes(b"".join(items), lens, len(items), buf, need.value, ctypes.byref(need)) == 0
        return buf.raw
    checked = 0
    for rec in G["fri"]:
        roots = [bytes.fromhex(h) for h in rec["roots"]]
        ps = ProofStream()
        for r, root in enumerate(roots):
            ps.push(root)
            raw = c_transcript(roots[:r + 1])
            assert raw == ps.serialize()
            out = ctypes.create_string_buffer(32)
            lib.sc_shake256(raw, len(raw), out, 32)
            assert out.raw == ps.prover_fiat_shamir()
            got = (ctypes.c_uint64 * 2)()
            lib.sc_field_sample(out.raw, 32, got)
            assert got[0] | (got[1] << 64) == field.sample(ps.prover_fiat_shamir()).value
            checked += 1
        # the challenge the indices are drawn from: over the roots and the last codeword (stored in full up to 64 elements)
        if rec["last_codeword"] is not None:
            last = [FieldElement(int(v), field) for v in rec["last_codeword"]]
            assert hashlib.sha256(synth.pack_ints([x.value for x in last])).hexdigest() == rec["last_codeword_sha256"]
            ps.push(last)
            assert ps.prover_fiat_shamir().hex() == rec["indices_seed"]
    assert checked == sum(r["num_rounds"] for r in G["fri"]) >= 100


def test_library_index_sampling_with_the_new_shapes():
    import starkcore
    lib = starkcore.lib()
    for rec in G["fri"]:
        n, s = 1 << rec["logN"], rec["num_colinearity_tests"]
        seed = bytes.fromhex(rec["indices_seed"])
        got = (ctypes.c_uint64 * s)()
        assert lib.sc_fri_sample_indices(seed, 32, n // 2, rec["last_codeword_len"], s, got) == 0
        assert list(got) == rec["top_level_indices"], (rec["logN"], rec["expansion_factor"], s)
        fr = Fri(field.generator(), field.primitive_nth_root(n), n, rec["expansion_factor"], s)
        assert fr.sample_indices(seed, n // 2, rec["last_codeword_len"], s) == rec["top_level_indices"]


def test_instances_have_the_recorded_shapes():
    from fast_stark import FastStark
    for rec in G["stark"]:
        ef, s = rec["expansion_factor"], rec["num_colinearity_checks"]
        if rec["kind"] == "rescue_prime":
            continue
        make = expansion_cases.synthetic_instance if rec["kind"] == "synthetic" else lambda *a: expansion_cases.wide_instance(a[0], rec["registers"], *a[1:])
        _, T, packed, rows, air, boundary = make(rec["log_fri"], ef, s)
        assert T == rec["original_trace_length"] == len(rows) and len(packed) == rec["registers"] == len(air)
        stark = FastStark(field, ef, s, rec["security_level"], rec["registers"], T)
        assert (stark.omicron_domain_length, stark.fri_domain_length) == (rec["omicron_domain_length"], rec["fri_domain_length"])
        assert stark.fri_domain_length == 1 << rec["log_fri"] == stark.omicron_domain_length * ef
        # the recorded alterations sit where alteration_places puts them, and one leaf and one path are at a companion position index + ef
        places = expansion_cases.alteration_places(rec["num_objects"], rec["registers"], ef, stark.fri_domain_length, rec["top_level_indices"])
        assert [{k: v for k, v in a.items() if k != "verifies"} for a in rec["alterations"]] == places
        companions = [a for a in places if a.get("companion_of") is not None and a["position"] == (a["companion_of"] + ef) % stark.fri_domain_length]
        assert {a["how"] == "add one" for a in companions} == {True, False}
