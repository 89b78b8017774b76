"""SynthesisError mirror (reference: src/lib.rs:303-319) + C-ABI return-code mapping."""

from ._abi import C


class SynthesisError(Exception):
    pass


class UnexpectedIdentity(SynthesisError):
    """src/multiexp.rs:63-65"""


class UnexpectedEof(SynthesisError, IOError):
    """io::ErrorKind::UnexpectedEof: `SynthesisError::IoError` "expected more bases from source" from multiexp
    (src/multiexp.rs:55-61) and the plain `io::Error` of a truncated `Parameters::read` / `VerifyingKey::read`
    (groth16/src/lib.rs:159-215,289-398) - so it is both a SynthesisError and an IOError."""


class PolynomialDegreeTooLarge(SynthesisError):
    """src/domain.rs:57-59"""


class UnconstrainedVariable(SynthesisError):
    """groth16/src/generator.rs:464-470"""


class Unsatisfiable(SynthesisError):
    """src/lib.rs:310: a witness does not satisfy a constraint of the circuit (prove_witness_batch(check=True));
    `.index` is the first unsatisfied constraint where the caller knows it"""

    def __init__(self, index=None):
        super().__init__("unsatisfiable constraint system" if index is None else "constraint %d is not satisfied" % index)
        self.index = index


class InvalidData(IOError):
    """io::ErrorKind::InvalidData from Parameters::read / VerifyingKey::read (groth16/src/lib.rs:159-215,289-398)"""


class InvalidPoint(InvalidData):
    """"invalid G1" / "invalid G2": bad encoding, or (checked) not on the curve / not in the subgroup"""


class PointAtInfinity(InvalidData):
    """"point at infinity": a query or ic point is the identity"""


class InvalidTranscript(Exception):
    """bh_powers_of_tau_verify: the transcript's vectors are not consistent powers of one (tau, alpha, beta).  `.report` is
    the ceremony.PtauReport of the call: `.failed` holds the BH_PTAU_FAILED_* bits of the equations that do not hold.
    bh_groth16_params_verify_step (Parameters.verify_step): `after` is not `before` with only delta rescaled; `.report` is
    the groth16.ParamsStepReport with the BH_STEP_FAILED_* bits."""

    def __init__(self, report=None, what="inconsistent powers-of-tau transcript"):
        super().__init__("%s (failed = 0x%02x)" % (what, report.failed if report is not None else 0))
        self.report = report


class BellmanHipError(RuntimeError):
    """HIP runtime failure / missing device: never silently replaced by a CPU path."""


def check(rc, what="bellman_hip call"):
    if rc == C.BH_OK:
        return
    if rc == C.BH_ERR_UNEXPECTED_IDENTITY:
        raise UnexpectedIdentity()
    if rc == C.BH_ERR_UNEXPECTED_EOF:
        raise UnexpectedEof("expected more bases from source")
    if rc == C.BH_ERR_DEGREE_TOO_LARGE:
        raise PolynomialDegreeTooLarge()
    if rc == C.BH_ERR_UNCONSTRAINED_VARIABLE:
        raise UnconstrainedVariable()
    if rc == C.BH_ERR_INVALID_POINT:
        raise InvalidPoint("invalid G1/G2")
    if rc == C.BH_ERR_POINT_AT_INFINITY:
        raise PointAtInfinity("point at infinity")
    if rc == C.BH_ERR_INVALID_TRANSCRIPT:
        raise InvalidTranscript()
    if rc == C.BH_ERR_UNSATISFIABLE:
        raise Unsatisfiable()
    if rc == C.BH_ERR_INVALID_ARG:
        # the reference panics here (assert!), e.g. src/multiexp.rs:324-329, src/domain.rs:155,174
        raise AssertionError("%s: invalid argument (the reference panics)" % what)
    if rc == C.BH_ERR_NO_DEVICE:
        raise BellmanHipError("%s: no gfx950 device available (no CPU fallback)" % what)
    raise BellmanHipError("%s failed with code %d" % (what, rc))


class VerificationError(Exception):
    """bellman::VerificationError (src/lib.rs:353-358)"""


class InvalidVerifyingKey(VerificationError):
    """the number of public inputs does not match the verifying key's ic (groth16/src/verifier.rs:27-29)"""


class InvalidProof(VerificationError):
    """the pairing equation does not hold (groth16/src/verifier.rs:55-57, verifier/batch.rs:186-190)"""


def check_verification(rc, what="verification"):
    """the return code of bh_groth16_verify / bh_groth16_batch_verify"""
    if rc == C.BH_ERR_INVALID_VERIFYING_KEY:
        raise InvalidVerifyingKey()
    if rc == C.BH_ERR_INVALID_PROOF:
        raise InvalidProof()
    check(rc, what)
