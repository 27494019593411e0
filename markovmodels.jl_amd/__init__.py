"""markovmodels.jl_amd -- MI355X-native engine behind MarkovModels.jl's inference API.

Host-side mirror of the reference's hot-path interface (src/MarkovModels.jl:14-45:
FSM, nstates, rawunion, CompiledFSM, batch, compile, expand, alpha-recursion,
beta-recursion, pdfposteriors, leakyposteriors, filterposteriors, windowposteriors, chunkedposteriors, windowbestpath, classbestpath, lattice, latticeposteriors, latticecost, latticebest, latticesample, arcposteriors, arcclassposteriors, scoredposteriors, classcost, weightedposteriors, samplepaths, expectedcost, pathentropy, totalsum, totalcumsum, totalweightsum) over the C ABI in include/markovmodels_amd.h.
The directory name contains a dot, so load it with
``__graft_entry__.load_package()`` (importlib) rather than a plain import.
"""
from ._lib import LIB_PATH, SYMBOLS, DimensionMismatch, MarkovModelsAMDError  # noqa: F401
from .fsm import FSM, GeneralStateMap, StateMap, arc_classes_by_destination, boundary_classes, loop_exit_classes, nstates, rawunion, statemap  # noqa: F401
from .inference import (  # noqa: F401
    BatchedFSM,
    CompiledFSM,
    Lattice,
    LatticeBest,
    LatticeCost,
    LatticePosteriors,
    LatticeSamples,
    alpharecursion,
    arcclassposteriors,
    arcposteriors,
    batch,
    bestpath,
    betarecursion,
    chunkedposteriors,
    classbestpath,
    compile,
    compile_many,
    compiled_cache_clear,
    compiled_cache_stats,
    expand,
    expectedcost,
    filterposteriors,
    lattice,
    latticebest,
    latticecost,
    latticeposteriors,
    latticesample,
    leakyposteriors,
    maxstateposteriors,
    pathentropy,
    pdfposteriors,
    samplepaths,
    scoredposteriors,
    classcost,
    totalcumsum,
    totalsum,
    totalweightsum,
    windowbestpath,
    weightedposteriors,
    windowposteriors,
    αrecursion,
    βrecursion,
)
from . import dist, linalg  # noqa: F401
from .linalg import SparseCSR, SparseVector, eldiv_, elmul_, mul_  # noqa: F401
from .lfmmi import lfmmi_loss  # noqa: F401
from .mbr import expected_class_cost, expected_cost, mpe_loss, smbr_loss  # noqa: F401
from . import entropy  # noqa: F401
from .entropy import conditional_entropy_loss, path_entropy  # noqa: F401
from . import graphweights  # noqa: F401
from .graphweights import graph_loglik, reestimate  # noqa: F401
from . import longform  # noqa: F401
from .longform import chunked_loglik  # noqa: F401
from . import transitions  # noqa: F401
from .transitions import constraint_scores, transition_loglik  # noqa: F401
from . import decode  # noqa: F401
from .decode import events, forced_alignment, lattice_arcs, lattice_fsm, lattice_onebest, lattice_prune, lattice_rescore, segments  # noqa: F401
from . import lattices  # noqa: F401
from .lattices import lattice_best_score, lattice_loglik, lattice_risk, lattice_sampled_risk, lattice_smbr_loss, pdf_costs, record_index  # noqa: F401
from . import streaming  # noqa: F401
from .streaming import FixedLagSmoother, ForwardFilter, OnlineViterbi  # noqa: F401
