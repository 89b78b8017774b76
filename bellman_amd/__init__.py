"""bellman_amd - MI355X (gfx950) implementation of bellman's Groth16 proving hot path.

Python host mirror of the reference's interface for the path (names and argument meaning follow
/root/reference/src/{multicore,multiexp,domain}.rs), implemented over the C ABI in
include/bellman_hip.h.  All arithmetic runs in hand-written HIP kernels (bellman_amd/csrc);
there is no CPU fallback - importing works without a GPU, creating a `Worker` does not.
"""

from .errors import (  # noqa: F401
    BellmanHipError,
    InvalidData,
    InvalidPoint,
    InvalidProof,
    InvalidTranscript,
    InvalidVerifyingKey,
    PointAtInfinity,
    PolynomialDegreeTooLarge,
    SynthesisError,
    UnconstrainedVariable,
    UnexpectedEof,
    UnexpectedIdentity,
    Unsatisfiable,
    VerificationError,
)
from .multicore import Waiter, Worker  # noqa: F401
from .multiexp import Bases, DensityTracker, FullDensity, Scalars, multiexp, multiexp_scalars, multiexp_sharded, point_add  # noqa: F401
from .multiexp import MANY_FORCE, multiexp_many  # noqa: F401
from .domain import EvaluationDomain, EvaluationDomains, PointEvaluationDomain, h_poly_many  # noqa: F401
from . import verifier  # noqa: F401,E402
from .verifier import (KeySet, MultiVerifier, PreparedVerifyingKey, Verifier, prepare_verifying_key, verify_each,  # noqa: F401,E402
                       verify_each_keys, verify_proof)
from . import ceremony  # noqa: F401,E402
from .ceremony import PtauReport, pairing_product_is_one, verify_powers_of_tau  # noqa: F401,E402
from .ceremony import bases_first_difference, contribute, same_ratio_each, tau_is_root_of_unity, verify_contributions  # noqa: F401,E402
from .ceremony import PowersOfTau, contribute_powers_of_tau, new_powers_of_tau, verify_powers_of_tau_update  # noqa: F401,E402
from .multiexp import point_mul_each  # noqa: F401,E402
from .groth16 import BitsHint, InverseOrZeroHint  # noqa: F401,E402
