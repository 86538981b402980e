"""The tutorial's signature scheme: Rescue-Prime STARK signatures (interface of reference code/fast_rpsss.py:1-73).

`SignatureProofStream(document)` and `FastRPSSS()` with `stark_prove`, `stark_verify`, `keygen`, `sign` and `verify`, at the
reference's parameters (expansion factor 4, 64 colinearity checks, security level 128, transition constraints of degree 3).  A
signature is a FastStark proof that the signer knows a preimage sk of pk = RescuePrime.hash(sk), with the Fiat-Shamir transcript
prefixed by the document's BLAKE2s digest.  With the same os.urandom the signature bytes are the reference's.

Added: `sign` computes the trace and the public output with one launch of the Rescue-Prime kernel (RescuePrime.trace_device);
`keygen_batch` / `keygen_batch_device` make many key pairs with one hash launch; `verify_batch` checks many signatures with one
FastStark.verify_batch call; `sign_batch` / `stark_prove_batch` make many signatures with one FastStark.prove_batch call.
"""
import os
import pickle
from hashlib import blake2s, shake_256

from algebra import Field
from ip import ProofStream
from fast_stark import FastStark, os_urandom_is_genuine
from rescue_prime import RescuePrime


class SignatureProofStream(ProofStream):
    def __init__(self, document):
        ProofStream.__init__(self)
        self.document = document
        self.prefix = blake2s(bytes(document)).digest()

    def prover_fiat_shamir(self, num_bytes=32):
        return shake_256(self.prefix + self.serialize()).digest(num_bytes)

    def verifier_fiat_shamir(self, num_bytes=32):
        return shake_256(self.prefix + pickle.dumps(self.objects[:self.read_index])).digest(num_bytes)

    def deserialize(self, bb):
        sps = SignatureProofStream(self.document)
        sps.objects = pickle.loads(bb)
        return sps


class FastRPSSS:
    # sign: the trace from the Rescue-Prime kernel (True) or the host mirror (False); both give the same signature
    SIGN_ON_DEVICE = True

    def __init__(self, num_colinearity_checks=64, grinding_bits=0, row_commitments=False, pair_leaves=False):
        """the defaults are the reference's parameters; fewer colinearity checks with as many grinding bits as keep 2 * checks + bits
        at the security level of 128 (FastStark(grinding_bits), grinding.py) give shorter signatures for a proof of work per signature.
        row_commitments: FastStark's option of the same name (one Merkle tree over the rows of the committed codewords), passed through
        pair_leaves: FastStark's option of the same name (FRI opens one pair and one path per colinearity test), passed through"""
        self.field = Field.main()
        expansion_factor = 4
        security_level = 128
        self.rp = RescuePrime()
        num_cycles = self.rp.N + 1
        state_width = self.rp.m
        self.stark = FastStark(self.field, expansion_factor, num_colinearity_checks, security_level, state_width, num_cycles,
                               transition_constraints_degree=3, grinding_bits=grinding_bits, row_commitments=row_commitments, pair_leaves=pair_leaves)
        self.transition_zerofier, self.transition_zerofier_codeword, self.transition_zerofier_root = self.stark.preprocess()

    def stark_prove(self, input_element, proof_stream):
        output_element = self.rp.hash(input_element)
        trace = self.rp.trace(input_element)
        return self._prove(trace, output_element, proof_stream)

    def _prove(self, trace, output_element, proof_stream):
        transition_constraints = self.rp.transition_constraints(self.stark.omicron)
        boundary_constraints = self.rp.boundary_constraints(output_element)
        return self.stark.prove(trace, transition_constraints, boundary_constraints, self.transition_zerofier,
                                self.transition_zerofier_codeword, proof_stream)

    def stark_verify(self, output_element, stark_proof, proof_stream):
        boundary_constraints = self.rp.boundary_constraints(output_element)
        transition_constraints = self.rp.transition_constraints(self.stark.omicron)
        return self.stark.verify(stark_proof, transition_constraints, boundary_constraints, self.transition_zerofier_root, proof_stream)

    def keygen(self):
        sk = self.field.sample(os.urandom(17))
        pk = self.rp.hash(sk)
        return sk, pk

    def keygen_batch_device(self, count):
        """`count` key pairs as two DeviceVectors (secret keys, public keys), the public keys from one hash launch.  With the operating
        system's os.urandom the library draws the secret keys (17 bytes each, Field.sample); a patched os.urandom is called key by
        key, so the pairs are those of `count` calls of keygen()."""
        import starkcore as sc
        sks = sc.DeviceVector(count)
        if count:
            if os_urandom_is_genuine():
                sc._check(sc.lib().sc_sample_urandom_dev(count, 17, sks.ptr, None))
            else:
                raw = b"".join(os.urandom(17) for _ in range(count))
                sc._check(sc.lib().sc_sample_bytes_dev(raw, count, 17, sks.ptr, None))
        return sks, self.rp.hash_device(sks)

    def keygen_batch(self, count):
        """([sk], [pk]) of `count` key pairs (see keygen_batch_device)"""
        import starkcore as sc
        from algebra import FieldElement
        sks, pks = self.keygen_batch_device(count)
        if not count:
            return [], []
        wrap = lambda vec: [FieldElement(v, self.field) for v in sc.unpack(vec.to_bytes())]
        return wrap(sks), wrap(pks)

    def sign(self, sk, document):
        sps = SignatureProofStream(document)
        if not self.SIGN_ON_DEVICE:
            return self.stark_prove(sk, sps)
        trace = self.rp.trace_device(sk)
        return self._prove(trace, trace.entry(self.rp.N, 0), sps)

    def sign_batch(self, sks, documents):
        """[self.sign(sk, document) for ...] -- the same signatures under the same os.urandom -- with one launch of the Rescue-Prime
        kernel for all traces, one gather of the public outputs and one FastStark.prove_batch"""
        sks, documents = list(sks), list(documents)
        assert len(sks) == len(documents), "one document per secret key"
        return self.stark_prove_batch(sks, [SignatureProofStream(document) for document in documents])

    def stark_prove_batch(self, input_elements, proof_streams):
        """the proofs of sign_batch on the caller's proof streams, one per input element"""
        import starkcore as sc
        from algebra import FieldElement
        from fast_stark import DeviceTrace
        input_elements, proof_streams = list(input_elements), list(proof_streams)
        assert len(input_elements) == len(proof_streams), "one proof stream per input element"
        if not input_elements:
            return []
        rows, m = self.rp.N + 1, self.rp.m
        # register s of input k's trace is column (m k + s) of one matrix: prove_batch reads the traces where they lie
        whole = self.rp.trace_batch_device(sc.DeviceVector.from_bytes(sc.pack([e.value % self.rp.p for e in input_elements])))
        base = whole.ptr
        traces = [DeviceTrace([sc.DeviceVector.wrap(base + 16 * rows * (m * k + s), rows, whole) for s in range(m)], self.field)
                  for k in range(len(input_elements))]
        outputs = whole.gather([rows * m * k + self.rp.N for k in range(len(input_elements))])      # register 0 at cycle N
        transition_constraints = self.rp.transition_constraints(self.stark.omicron)
        boundaries = [self.rp.boundary_constraints(FieldElement(v, self.field)) for v in outputs]
        return self.stark.prove_batch(traces, transition_constraints, boundaries, self.transition_zerofier, self.transition_zerofier_codeword,
                                      proof_streams)

    def verify(self, pk, document, signature):
        sps = SignatureProofStream(document)
        return self.stark_verify(pk, signature, sps)

    def verify_batch(self, pks, documents, signatures):
        """[self.verify(pk, document, signature) ...] in one FastStark.verify_batch call (every Merkle path and colinearity test of
        the batch on the device at once); a malformed signature is reported False"""
        pks, documents, signatures = list(pks), list(documents), list(signatures)
        assert len(pks) == len(documents) == len(signatures), "one public key and one document per signature"
        if not signatures:
            return []
        transition_constraints = self.rp.transition_constraints(self.stark.omicron)
        boundaries = [self.rp.boundary_constraints(pk) for pk in pks]
        streams = [SignatureProofStream(document) for document in documents]
        return self.stark.verify_batch(signatures, transition_constraints, boundaries, self.transition_zerofier_root, streams)
