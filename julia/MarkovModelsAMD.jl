# SPDX-License-Identifier: MIT
#
# MarkovModelsAMD.jl -- the binding a MarkovModels.jl maintainer would add so that
# `pdfposteriors`, `αrecursion` and `βrecursion` run on an AMD MI355X through
# libmarkovmodels_amd.so (C ABI: include/markovmodels_amd.h).
#
# NOT TESTED IN THIS REPOSITORY: the build image has no Julia.  The tested binding
# of the same ABI is the Python/ctypes one in markovmodels.jl_amd/_lib.py; this file
# mirrors it call for call.  Device memory comes from AMDGPU.jl (ROCArray).
#
# `using MarkovModels` loads CUDA.jl (a hard dependency of the package: src/MarkovModels.jl:7-8); on an AMD box CUDA.jl
# loads without a device (CUDA.functional() == false) and nothing here calls into it.
#
# Seam (see INTEGRATION.md): the reference dispatches on CuArray storage
# (src/fsm.jl:42-48, src/inference.jl:14-26, src/linalg.jl:163,240,335).  Here the
# dispatch is on a device handle type, one level up: one ccall per inference call.

module MarkovModelsAMD

using MarkovModels
using SparseArrays
using Semirings
using AMDGPU
using Adapt
using Libdl
using LinearAlgebra

# The package's own generic functions are EXTENDED with methods for the device types below (`using MarkovModels`
# already exports compile, batch, pdfposteriors, ...: src/MarkovModels.jl:14-45 -- defining functions of the same
# names in this module would shadow them instead).
import MarkovModels: compile, batch, pdfposteriors, αrecursion, βrecursion, totalsum, totalcumsum

# what this module adds to the package's API
export ROCCompiledFSM, ROCBatch, to_device, compile_many, bestpath, maxstateposteriors, arcposteriors, set_arc_classes!, arc_class_info, arcclassposteriors, score_class_cap, scoredposteriors, cost_class_cap, classcost, weightedposteriors, samplepaths, expectedcost, pathentropy, leakyposteriors, filterposteriors, windowposteriors, segmentposteriors, viterbiwindow, set_path_classes!, path_class_info, classpath, lattice, latticeposteriors, latticecost, latticebest, latticesample, pdfposteriors_generic, last_redo_count,
       last_fallback_count, last_exact_first, team_xcd_stats, reserve_ex!, set_deterministic!, set_posterior_floor!, set_exact_policy!,
       set_mark_policy!, set_gamma_mode!, set_rccl, allreduce_logz, allgather_ttl, ROCSparseCSR, ROCSparseVec, elmul!, eldiv!,
       compiled_cache_clear!, compiled_cache_limits!

const LIB = get(ENV, "MARKOVMODELS_AMD_LIB", "libmarkovmodels_amd.so")

const MM_LOG, MM_TROPICAL, MM_PROB = Cint(0), Cint(1), Cint(2)
const MM_CSC = Cint(0)
const MM_ABI_VERSION = 4      # include/markovmodels_amd.h: the version every ccall tuple of this file was written against

# A library of another ABI version would be called with the wrong argument lists: refuse it when the module is loaded.
function __init__()
    v = ccall((:mm_abi_version, LIB), Cint, ())
    v == MM_ABI_VERSION || error("$(LIB) has ABI version $(v), MarkovModelsAMD.jl was written against $(MM_ABI_VERSION)")
    nothing
end

struct MMError <: Exception
    code::Cint
    msg::String
end

function check(rc::Cint)
    rc == 0 && return
    msg = unsafe_string(ccall((:mm_last_error, LIB), Cstring, ()))
    rc == -2 && throw(DimensionMismatch(msg))      # src/linalg.jl:166-167
    throw(MMError(rc, msg))
end

semiring_id(::Type{<:LogSemiring}) = MM_LOG
semiring_id(::Type{<:TropicalSemiring}) = MM_TROPICAL
semiring_id(::Type{<:ProbSemiring}) = MM_PROB      # the generic entry only (pdfposteriors_generic)

"Device-resident compiled FSM: replaces adapt(CuArray, ::CompiledFSM) (src/inference.jl:14-26)."
mutable struct ROCCompiledFSM{K}
    handle::Ptr{Cvoid}
    S1::Int
    P1::Int
end

"""
    compile(ROCCompiledFSM, fsm, Ĉ)

`compile(fsm, Ĉ)` (src/inference.jl:11-12) + device adapt.  `Ĉ` is the state map
of examples/prepare-lfmmi-graphs.jl:15-23 (exactly one stored entry per row).
"""
compile(::Type{ROCCompiledFSM}, fsm::FSM{K}, Ĉ::AbstractSparseMatrix) where K =
    _create(K, SparseMatrixCSC(fsm.T̂), SparseVector(fsm.α̂), Ĉ)

"""
    to_device(cfsm::CompiledFSM) -> ROCCompiledFSM

What `adapt(CuArray, cfsm)` / `cfsm |> gpu` is on the CUDA path (src/inference.jl:14-26): the compiled FSM of the
reference, as `compile(fsm, Ĉ)` made it on the host, handed to the engine.  `batch(to_device(c)...)` then replaces
`batch(c...) |> gpu`.
"""
to_device(c::CompiledFSM{K}) where K = _create(K, SparseMatrixCSC(c.T̂), SparseVector(c.α̂), c.Ĉ)

"""
    Adapt.adapt_structure(ROCArray, cfsm::CompiledFSM) -> ROCCompiledFSM

The reference's own seam (src/inference.jl:14-26: `adapt_structure(::Type{<:CuArray}, cfsm)`, reached through
`cfsm |> gpu` / `adapt(CuArray, cfsm)`): `adapt(ROCArray, cfsm)` hands the compiled FSM to the engine.  The FSM type
itself (src/fsm.jl:42-48) has no device form here: the engine takes compiled FSMs (`compile(fsm, Ĉ)` first).
"""
Adapt.adapt_structure(::Type{<:ROCArray}, c::CompiledFSM) = to_device(c)

"""
    compile_many(fsms::Vector{FSM{K}}, Ĉs) -> Vector{ROCCompiledFSM{K}}

`compile.(fsms, Ĉs)` + device adapt for a mini-batch of NEW graphs in one call (mm_fsm_create_many: host threads, one device
allocation, one copy) -- what examples/test_cuda.jl:74-78 does every training step for the numerator graphs.
"""
function compile_many(fsms::Vector{<:FSM{K}}, Ĉs::Vector{<:AbstractSparseMatrix}; threads::Integer = 0) where K
    n = length(fsms)
    n == length(Ĉs) || throw(DimensionMismatch("one Ĉ per FSM"))
    Ts = [SparseMatrixCSC(f.T̂) for f in fsms]
    αs = [SparseVector(f.α̂) for f in fsms]
    vals = [val.(nonzeros(T)) for T in Ts]
    avals = [val.(nonzeros(a)) for a in αs]
    ainds = [SparseArrays.nonzeroinds(a) for a in αs]
    s2ps = map(Ĉs) do Ĉ
        Ct = SparseMatrixCSC(copy(Ĉ'))
        all(diff(Ct.colptr) .== 1) || throw(ArgumentError("Ĉ must have exactly one entry per row"))
        Vector{Int32}(Ct.rowval)
    end
    F = eltype(vals[1])
    S1 = Int64[size(T, 1) for T in Ts]
    NZ = Int64[nnz(T) for T in Ts]
    NI = Int64[nnz(a) for a in αs]
    P1 = Int32[size(Ĉ, 2) for Ĉ in Ĉs]
    out = fill(Ptr{Cvoid}(C_NULL), n)
    GC.@preserve Ts αs vals avals ainds s2ps begin
        p_ptr = Ptr{Cvoid}[pointer(T.colptr) for T in Ts]
        p_idx = Ptr{Cvoid}[pointer(T.rowval) for T in Ts]
        p_val = Ptr{Cvoid}[pointer(v) for v in vals]
        p_ai = Ptr{Cvoid}[pointer(a) for a in ainds]
        p_av = Ptr{Cvoid}[pointer(a) for a in avals]
        p_s2p = Ptr{Int32}[pointer(s) for s in s2ps]
        check(ccall((:mm_fsm_create_many, LIB), Cint,
            (Int64, Cint, Cint, Cint, Cint, Cint, Ptr{Int64}, Ptr{Int64}, Ptr{Ptr{Cvoid}}, Ptr{Ptr{Cvoid}}, Ptr{Ptr{Cvoid}},
             Ptr{Int64}, Ptr{Ptr{Cvoid}}, Ptr{Ptr{Cvoid}}, Ptr{Ptr{Int32}}, Ptr{Int32}, Cint, Ptr{Ptr{Cvoid}}),
            n, semiring_id(K), MM_CSC, 8, 1, sizeof(F), S1, NZ, p_ptr, p_idx, p_val, NI, p_ai, p_av, p_s2p, P1, threads, out))
    end
    map(1:n) do i
        obj = ROCCompiledFSM{K}(out[i], S1[i], P1[i])
        finalizer(o -> ccall((:mm_fsm_destroy, LIB), Cint, (Ptr{Cvoid},), o.handle), obj)
        obj
    end
end

function _create(::Type{K}, T̂::SparseMatrixCSC, α̂::SparseVector, Ĉ::AbstractSparseMatrix) where K
    Ct = SparseMatrixCSC(copy(Ĉ'))                      # column s of Ĉ' = row s of Ĉ
    all(diff(Ct.colptr) .== 1) || throw(ArgumentError("Ĉ must have exactly one entry per row"))
    state2pdf = Vector{Int32}(Ct.rowval)                # 1-based pdf of every state
    vals = val.(nonzeros(T̂))
    avals = val.(nonzeros(α̂))
    T = eltype(vals)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve T̂ α̂ state2pdf vals avals begin
        check(ccall((:mm_fsm_create, LIB), Cint,
            (Cint, Int64, Int64, Cint, Cint, Cint, Cint, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Int64,
             Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Int32}, Int32, Ref{Ptr{Cvoid}}),
            semiring_id(K), size(T̂, 1), nnz(T̂), MM_CSC, 8, 1, sizeof(T),
            pointer(T̂.colptr), pointer(T̂.rowval), pointer(vals), nnz(α̂),
            pointer(SparseArrays.nonzeroinds(α̂)), pointer(avals), pointer(state2pdf),
            Int32(size(Ĉ, 2)), h))
    end
    obj = ROCCompiledFSM{K}(h[], size(T̂, 1), size(Ĉ, 2))
    finalizer(o -> ccall((:mm_fsm_destroy, LIB), Cint, (Ptr{Cvoid},), o.handle), obj)
    obj
end

"batch(cfsm...) (src/inference.jl:28-36); repeating one handle shares its storage."
mutable struct ROCBatch{K}
    handle::Ptr{Cvoid}
    fsms::Vector{ROCCompiledFSM{K}}      # keeps the FSM handles alive
    P::Int
    keep::Any                            # device arrays an asynchronous call on this batch still reads (replaced by the next call)
end

function batch(f1::ROCCompiledFSM{K}, fs::ROCCompiledFSM{K}...) where K
    all_ = ROCCompiledFSM{K}[f1, fs...]
    hs = Ptr{Cvoid}[f.handle for f in all_]
    h = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:mm_batch_create, LIB), Cint, (Ptr{Ptr{Cvoid}}, Int64, Ref{Ptr{Cvoid}}), hs, length(hs), h))
    obj = ROCBatch{K}(h[], all_, f1.P1 - 1, nothing)
    finalizer(o -> ccall((:mm_batch_destroy, LIB), Cint, (Ptr{Cvoid},), o.handle), obj)
    obj
end

"""
    pdfposteriors(b::ROCBatch, V::ROCArray{Float32,3}, lens)

Drop-in for pdfposteriors(fsm, V̂s, Ĉs) (src/inference.jl:145-161) /
pdfposteriors2 (:164-180).  `V` is P × N × B (Julia column-major: pdf fastest, the
layout of `vcat(V̂s...)` without the phony row/frame: expand() happens inside);
`lens` a ROCVector{Int32} or nothing.  Returns (γ::ROCArray{Float32,3} of size
B × P × N like the reference, ttl::ROCVector{Float32}).
"""
function pdfposteriors(b::ROCBatch, V::ROCArray{Float32,3}, lens = nothing; out::Union{Nothing, ROCArray{Float32,3}} = nothing)
    P, N, B = size(V)
    P == b.P || throw(DimensionMismatch("V has $P pdfs, the FSMs $(b.P)"))
    out === nothing || size(out) == (B, P, N) || throw(DimensionMismatch("out must be B × P × N"))
    γ = out === nothing ? ROCArray{Float32}(undef, B, P, N) : out      # (`out`: the array set_gamma_mode!(accumulate = true) adds into)
    ttl = ROCArray{Float32}(undef, B)
    lp = lens === nothing ? Ptr{Int32}(C_NULL) : Ptr{Int32}(pointer(lens))
    # strides in elements: V (b, n, p) -> p + P*n + P*N*b ; γ (b, n, p) -> b + B*p + B*P*n
    check(ccall((:mm_pdfposteriors_f32, LIB), Cint,
        (Ptr{Cvoid}, Ptr{Float32}, Int64, Int64, Ptr{Int32}, Int64, Ptr{Float32}, Int64, Int64, Int64,
         Ptr{Float32}, Ptr{Cvoid}),
        b.handle, pointer(V), P * N, P, lp, N, pointer(γ), 1, B * P, B, pointer(ttl),
        AMDGPU.stream().stream))
    γ, ttl
end

"""
    arcposteriors(b::ROCBatch, V::ROCArray{Float32,3}, fsms, lens = nothing) -> (counts, init, ttl)

Expected arc counts (mm_arcposteriors_f32 in the header: Baum-Welch's ξ summed over the frames) of a log-semiring batch.  `V`
and `lens` as for `pdfposteriors`; `fsms` the FSMs the batch was compiled from, in its order (their patterns).  Returns, per
utterance, a `SparseMatrixCSC` with the pattern of its `T̂` holding the counts (phony final column and self-loop included:
the counts of an utterance with a path sum to N), the expected initial-state occupancy as a `SparseVector` with the
pattern of its `α̂`, and ttl = log Z (a `Vector{Float32}`).  `counts[i, j]` is also ∂ log Z / ∂ log T̂[i, j].
"""
function arcposteriors(b::ROCBatch, V::ROCArray{Float32,3}, fsms::AbstractVector, lens = nothing)
    P, N, B = size(V)
    P == b.P || throw(DimensionMismatch("V has $P pdfs, the FSMs $(b.P)"))
    length(fsms) == B || throw(DimensionMismatch("$(length(fsms)) FSMs for a batch of $B utterances"))
    Ts = [SparseMatrixCSC(f.T̂) for f in fsms]      # (the entry order _create handed to mm_fsm_create: CSC)
    αs = [SparseVector(f.α̂) for f in fsms]
    K = maximum(nnz, Ts)
    I = max(1, maximum(nnz, αs))
    counts = ROCArray{Float32}(undef, K, B)          # utterance b's counts at column b: c_stride_b = K
    init = ROCArray{Float32}(undef, I, B)
    ttl = ROCArray{Float32}(undef, B)
    lp = lens === nothing ? Ptr{Int32}(C_NULL) : Ptr{Int32}(pointer(lens))
    check(ccall((:mm_arcposteriors_f32, LIB), Cint,
        (Ptr{Cvoid}, Ptr{Float32}, Int64, Int64, Ptr{Int32}, Int64, Ptr{Float32}, Int64, Ptr{Float32}, Int64,
         Ptr{Float32}, Ptr{Cvoid}),
        b.handle, pointer(V), P * N, P, lp, N, pointer(counts), K, pointer(init), I, pointer(ttl),
        AMDGPU.stream().stream))
    c, iv = Array(counts), Array(init)
    mats = [SparseMatrixCSC(size(T, 1), size(T, 2), copy(T.colptr), copy(T.rowval), c[1:nnz(T), u]) for (u, T) in enumerate(Ts)]
    inits = [SparseVector(length(a), copy(SparseArrays.nonzeroinds(a)), iv[1:nnz(a), u]) for (u, a) in enumerate(αs)]
    mats, inits, Array(ttl)
end

"""
    set_arc_classes!(b::ROCBatch, classes, C = nothing) -> C

The class of every stored entry of `T̂` for `arcclassposteriors` (mm_batch_set_arc_classes in the header): `classes` is one
`Vector{<:Integer}` of `nnz` ids for a batch of one shared FSM, or a vector with one such vector per utterance; ids in `-1:C-1`
(0-based, -1: not counted), in the CSC entry order of `SparseMatrixCSC(fsm.T̂)`.  Host work only; calling it again replaces the plan.
"""
function set_arc_classes!(b::ROCBatch, classes::AbstractVector, C = nothing)
    shared = !(eltype(classes) <: AbstractVector)
    parts = shared ? [classes] : classes
    flat = Int32[]
    offs = Int64[0]
    for c in parts
        append!(flat, Int32.(c))
        push!(offs, length(flat))
    end
    nc = C === nothing ? max(1, Int(maximum(flat; init = Int32(0))) + 1) : Int(C)
    op = shared ? Ptr{Int64}(C_NULL) : pointer(offs)
    GC.@preserve flat offs check(ccall((:mm_batch_set_arc_classes, LIB), Cint, (Ptr{Cvoid}, Ptr{Int32}, Ptr{Int64}, Int32),
        b.handle, pointer(flat), op, Int32(nc)))
    nc
end

"(cap, max_M, C) of the batch's arc-class plan (mm_batch_arc_class_info): the most classified entries whose terms stay in LDS, the most one utterance of the plan has (-1: no plan), the classes"
function arc_class_info(b::ROCBatch)
    cap, m, c = Ref{Int64}(0), Ref{Int64}(0), Ref{Int32}(0)
    check(ccall((:mm_batch_arc_class_info, LIB), Cint, (Ptr{Cvoid}, Ptr{Int64}, Ptr{Int64}, Ptr{Int32}), b.handle, cap, m, c))
    (cap = cap[], max_M = m[], C = Int(c[]))
end

"""
    arcclassposteriors(b::ROCBatch, V::ROCArray{Float32,3}, lens = nothing) -> (ξ, ttl)

Per-frame arc-class posteriors (mm_arcclassposteriors_f32 in the header; Baum-Welch's ξₙ summed by the classes of
`set_arc_classes!`): `ξ[c, t, u]` (a `C × N × B` array on the device) is the posterior probability that utterance u takes an arc
of class c - 1 between frames t and t + 1; frames beyond an utterance's length belong to the phony self-loop.
"""
function arcclassposteriors(b::ROCBatch, V::ROCArray{Float32,3}, lens = nothing)
    P, N, B = size(V)
    P == b.P || throw(DimensionMismatch("V has $P pdfs, the FSMs $(b.P)"))
    nc = max(1, arc_class_info(b).C)
    ξ = ROCArray{Float32}(undef, nc, N, B)
    ttl = ROCArray{Float32}(undef, B)
    lp = lens === nothing ? Ptr{Int32}(C_NULL) : Ptr{Int32}(pointer(lens))
    check(ccall((:mm_arcclassposteriors_f32, LIB), Cint,
        (Ptr{Cvoid}, Ptr{Float32}, Int64, Int64, Ptr{Int32}, Int64, Ptr{Float32}, Int64, Int64, Int64, Ptr{Float32}, Ptr{Cvoid}),
        b.handle, pointer(V), P * N, P, lp, N, pointer(ξ), nc * N, nc, 1, pointer(ttl), AMDGPU.stream().stream))
    ξ, ttl
end

"The most classes `scoredposteriors` takes on this batch (mm_batch_score_class_cap): their score rows fit the LDS beside the kernel's plan"
function score_class_cap(b::ROCBatch)
    cap = Ref{Int64}(0)
    check(ccall((:mm_batch_score_class_cap, LIB), Cint, (Ptr{Cvoid}, Ptr{Int64}), b.handle, cap))
    cap[]
end

"""
    scoredposteriors(b::ROCBatch, V::ROCArray{Float32,3}, U = nothing, lens = nothing) -> (γ, ξ, ttl)

Posteriors with per-frame arc-class scores (mm_scoredposteriors_f32 in the header): under the classes of `set_arc_classes!` the
entry taken between frames t and t + 1 is weighted by `exp(U[c, t, u])` on top of its own weight.  `U` is a `C × N × B`
`ROCArray{Float32,3}` (finite or `-Inf`), `nothing`: no scores.  `γ` (`P × N × B`) is ∂ log Z / ∂ V, `ξ` (`C × N × B`) is
∂ log Z / ∂ U on the frames below an utterance's length and what `arcclassposteriors` returns beyond, `ttl` = log Z(U).
"""
function scoredposteriors(b::ROCBatch, V::ROCArray{Float32,3}, U = nothing, lens = nothing)
    P, N, B = size(V)
    P == b.P || throw(DimensionMismatch("V has $P pdfs, the FSMs $(b.P)"))
    nc = max(1, arc_class_info(b).C)
    U === nothing || size(U) == (nc, N, B) || throw(DimensionMismatch("U must be $nc × $N × $B"))
    γ = ROCArray{Float32}(undef, P, N, B)
    ξ = ROCArray{Float32}(undef, nc, N, B)
    ttl = ROCArray{Float32}(undef, B)
    lp = lens === nothing ? Ptr{Int32}(C_NULL) : Ptr{Int32}(pointer(lens))
    up = U === nothing ? Ptr{Float32}(C_NULL) : Ptr{Float32}(pointer(U))
    check(ccall((:mm_scoredposteriors_f32, LIB), Cint,
        (Ptr{Cvoid}, Ptr{Float32}, Int64, Int64, Ptr{Int32}, Int64, Ptr{Float32}, Int64, Int64, Int64, Ptr{Float32}, Int64, Int64, Int64,
         Ptr{Float32}, Int64, Int64, Int64, Ptr{Float32}, Ptr{Cvoid}),
        b.handle, pointer(V), P * N, P, lp, N, up, nc * N, nc, 1, pointer(γ), P * N, P, 1, pointer(ξ), nc * N, nc, 1, pointer(ttl),
        AMDGPU.stream().stream))
    γ, ξ, ttl
end

"""
    weightedposteriors(b::ROCBatch, V::ROCArray{Float32,3}, fsms, W, lens = nothing; W_init = nothing) -> (γ, counts, init, ttl)

Posteriors with call-time arc weights (mm_weightedposteriors_f32 in the header) of a log-semiring batch: the topology and the
compiled forms stay the batch's, the arc log-weights of this call are `W` and the initial log-weights `W_init`, both on the
device.  `W` a `ROCVector{Float32}` is one weight vector for the whole batch (all utterances must be the same FSM), a
`ROCMatrix{Float32}` of nnz rows and B columns one per utterance, `nothing` the FSMs' own; the entries follow `nonzeros(T̂)`
(the order `counts` uses), `W_init` likewise follows `nonzeros(α̂)`.  `-Inf32` takes an entry out for this call; the phony
self-loop stays one(K).  Returns γ (P × N × B, as `pdfposteriors`), the counts and initial occupancies as `arcposteriors`
returns them, and ttl = log Z: `counts = ∂ log Z / ∂ W`, `init = ∂ log Z / ∂ W_init`, `γ = ∂ log Z / ∂ V`.
"""
function weightedposteriors(b::ROCBatch, V::ROCArray{Float32,3}, fsms::AbstractVector, W, lens = nothing; W_init = nothing)
    P, N, B = size(V)
    P == b.P || throw(DimensionMismatch("V has $P pdfs, the FSMs $(b.P)"))
    length(fsms) == B || throw(DimensionMismatch("$(length(fsms)) FSMs for a batch of $B utterances"))
    Ts = [SparseMatrixCSC(f.T̂) for f in fsms]
    αs = [SparseVector(f.α̂) for f in fsms]
    K = maximum(nnz, Ts)
    I = max(1, maximum(nnz, αs))
    wptr(w) = w === nothing ? Ptr{Float32}(C_NULL) : Ptr{Float32}(pointer(w))
    wstride(w, need) = (w === nothing || ndims(w) == 1) ? 0 :
        (size(w, 1) >= need && size(w, 2) == B ? size(w, 1) : throw(DimensionMismatch("weights must be $need × $B, got $(size(w))")))
    W === nothing || size(W, 1) >= K || throw(DimensionMismatch("W has $(size(W, 1)) entries, the largest FSM $K"))
    γ = ROCArray{Float32}(undef, B, P, N)
    counts = ROCArray{Float32}(undef, K, B)
    init = ROCArray{Float32}(undef, I, B)
    ttl = ROCArray{Float32}(undef, B)
    lp = lens === nothing ? Ptr{Int32}(C_NULL) : Ptr{Int32}(pointer(lens))
    check(ccall((:mm_weightedposteriors_f32, LIB), Cint,
        (Ptr{Cvoid}, Ptr{Float32}, Int64, Int64, Ptr{Int32}, Int64, Ptr{Float32}, Int64, Ptr{Float32}, Int64,
         Ptr{Float32}, Int64, Int64, Int64, Ptr{Float32}, Int64, Ptr{Float32}, Int64, Ptr{Float32}, Ptr{Cvoid}),
        b.handle, pointer(V), P * N, P, lp, N, wptr(W), wstride(W, K), wptr(W_init), wstride(W_init, maximum(nnz, αs)),
        pointer(γ), 1, B * P, B, pointer(counts), K, pointer(init), I, pointer(ttl), AMDGPU.stream().stream))
    c, iv = Array(counts), Array(init)
    mats = [SparseMatrixCSC(size(T, 1), size(T, 2), copy(T.colptr), copy(T.rowval), c[1:nnz(T), u]) for (u, T) in enumerate(Ts)]
    inits = [SparseVector(length(a), copy(SparseArrays.nonzeroinds(a)), iv[1:nnz(a), u]) for (u, a) in enumerate(αs)]
    permutedims(γ, (2, 3, 1)), mats, inits, Array(ttl)
end

"""
    samplepaths(b::ROCBatch, V::ROCArray{Float32,3}, lens = nothing; nsamples = 1, seed = 0) -> (paths, logprob, ttl)

State sequences drawn from the posterior over complete paths (mm_samplepaths_f32 in the header: forward filtering, backward
sampling) of a log-semiring batch.  `V` and `lens` as for `pdfposteriors`.  Returns `paths`, an N × nsamples × B `Array{Int32}`
of 1-based states (0 beyond an utterance's length, and everywhere for an utterance without a path), the natural-log posterior
probability of every sampled sequence (nsamples × B) and ttl = log Z.  A sample depends on the graphs, `V`, `lens`, `seed` and
its indices (utterance, sample) alone: the same `seed` gives the same samples, and the first K′ samples of a call with
`nsamples = K` are the samples of a call with `nsamples = K′`.
"""
function samplepaths(b::ROCBatch, V::ROCArray{Float32,3}, lens = nothing; nsamples::Integer = 1, seed::Integer = 0)
    P, N, B = size(V)
    P == b.P || throw(DimensionMismatch("V has $P pdfs, the FSMs $(b.P)"))
    K = Int64(nsamples)
    K >= 1 || throw(ArgumentError("nsamples must be at least 1"))
    paths = ROCArray{Int32}(undef, N, K, B)
    logprob = ROCArray{Float32}(undef, K, B)
    ttl = ROCArray{Float32}(undef, B)
    lp = lens === nothing ? Ptr{Int32}(C_NULL) : Ptr{Int32}(pointer(lens))
    check(ccall((:mm_samplepaths_f32, LIB), Cint,
        (Ptr{Cvoid}, Ptr{Float32}, Int64, Int64, Ptr{Int32}, Int64, Int64, Int64, Ptr{Int32}, Int64, Int64,
         Ptr{Float32}, Int64, Ptr{Float32}, Ptr{Cvoid}),
        b.handle, pointer(V), P * N, P, lp, N, K, seed % Int64, pointer(paths), N * K, N, pointer(logprob), K, pointer(ttl),
        AMDGPU.stream().stream))
    Array(paths) .+ Int32(1), Array(logprob), Array(ttl)      # (the library's states are 0-based, -1 = no state)
end

"""
    expectedcost(b::ROCBatch, V::ROCArray{Float32,3}, cost::ROCArray{Float32,3}, lens = nothing) -> (risk, grad, γ, ttl)

Expected cost of a path under the path posterior and its gradient (mm_expectedcost_f32 in the header) of a log-semiring batch.
`V` and `lens` as for `pdfposteriors`; `cost` laid out like `V` (P × N × B): what an utterance pays for a state of pdf p at frame
n (finite inside the length, not read beyond it).  Returns `risk` (B), `grad` = ∂ risk / ∂ V and `γ` = ∂ risk / ∂ cost (the pdf
posteriors), both B × P × N like `pdfposteriors`' γ, and ttl = log Z.  With `cost = -onehot(reference pdfs)` on the denominator
graph, `risk` is the lattice-free sMBR objective (minus the expected number of correct frames).
"""
function expectedcost(b::ROCBatch, V::ROCArray{Float32,3}, cost::ROCArray{Float32,3}, lens = nothing)
    P, N, B = size(V)
    P == b.P || throw(DimensionMismatch("V has $P pdfs, the FSMs $(b.P)"))
    size(cost) == size(V) || throw(DimensionMismatch("cost is $(size(cost)), V $(size(V))"))
    risk = ROCArray{Float32}(undef, B)
    grad = ROCArray{Float32}(undef, B, P, N)
    γ = ROCArray{Float32}(undef, B, P, N)
    ttl = ROCArray{Float32}(undef, B)
    lp = lens === nothing ? Ptr{Int32}(C_NULL) : Ptr{Int32}(pointer(lens))
    check(ccall((:mm_expectedcost_f32, LIB), Cint,
        (Ptr{Cvoid}, Ptr{Float32}, Int64, Int64, Ptr{Int32}, Int64, Ptr{Float32}, Int64, Int64,
         Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Int64, Int64, Int64, Ptr{Float32}, Ptr{Cvoid}),
        b.handle, pointer(V), P * N, P, lp, N, pointer(cost), P * N, P,
        pointer(risk), pointer(grad), pointer(γ), 1, B * P, B, pointer(ttl),
        AMDGPU.stream().stream))
    risk, grad, γ, ttl
end

"The most classes `classcost` takes on this batch (mm_batch_cost_class_cap): their cost rows fit the LDS behind the cost kernels' plan"
function cost_class_cap(b::ROCBatch)
    cap = Ref{Int64}(0)
    check(ccall((:mm_batch_cost_class_cap, LIB), Cint, (Ptr{Cvoid}, Ptr{Int64}), b.handle, cap))
    cap[]
end

"""
    classcost(b::ROCBatch, V::ROCArray{Float32,3}, A::ROCArray{Float32,3}, lens = nothing; D = nothing) -> (risk, grad, γ, ttl)

Expected arc-class cost under the path posterior and its gradient (mm_classcost_f32 in the header) of a log-semiring batch: under
the classes of `set_arc_classes!` the entry taken between frames t and t + 1 costs `A[c, t, u]` (`C × N × B`, finite inside the
length, not read beyond it); `D` (`P × N × B`, optional) are pdf costs as `expectedcost` takes them.  Returns `risk` (B),
`grad` = ∂ risk / ∂ V and `γ` = ∂ risk / ∂ D (the pdf posteriors), both B × P × N like `pdfposteriors`' γ, and ttl = log Z.
∂ risk / ∂ A is the ξ of `arcclassposteriors`.  With `A = -onehot(reference classes)` on the denominator graph, `risk` is the
lattice-free MPE objective (minus the expected number of correct arcs).
"""
function classcost(b::ROCBatch, V::ROCArray{Float32,3}, A::ROCArray{Float32,3}, lens = nothing; D = nothing)
    P, N, B = size(V)
    P == b.P || throw(DimensionMismatch("V has $P pdfs, the FSMs $(b.P)"))
    nc = max(1, arc_class_info(b).C)
    size(A) == (nc, N, B) || throw(DimensionMismatch("A must be $nc × $N × $B"))
    D === nothing || size(D) == size(V) || throw(DimensionMismatch("D is $(size(D)), V $(size(V))"))
    risk = ROCArray{Float32}(undef, B)
    grad = ROCArray{Float32}(undef, B, P, N)
    γ = ROCArray{Float32}(undef, B, P, N)
    ttl = ROCArray{Float32}(undef, B)
    lp = lens === nothing ? Ptr{Int32}(C_NULL) : Ptr{Int32}(pointer(lens))
    dp = D === nothing ? Ptr{Float32}(C_NULL) : Ptr{Float32}(pointer(D))
    check(ccall((:mm_classcost_f32, LIB), Cint,
        (Ptr{Cvoid}, Ptr{Float32}, Int64, Int64, Ptr{Int32}, Int64, Ptr{Float32}, Int64, Int64, Int64, Ptr{Float32}, Int64, Int64,
         Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Int64, Int64, Int64, Ptr{Float32}, Ptr{Cvoid}),
        b.handle, pointer(V), P * N, P, lp, N, pointer(A), nc * N, nc, 1, dp, P * N, P,
        pointer(risk), pointer(grad), pointer(γ), 1, B * P, B, pointer(ttl),
        AMDGPU.stream().stream))
    risk, grad, γ, ttl
end

"""
    pathentropy(b::ROCBatch, V::ROCArray{Float32,3}, lens = nothing; grad = true) -> (H, grad, γ, ttl)

Entropy of the posterior over complete paths, H_b = -Σ_π P(π | V_b) log P(π | V_b) in nats, and its gradient in the emissions
(mm_pathentropy_f32 in the header) of a log-semiring batch.  `V` and `lens` as for `pdfposteriors`.  Returns `H` (B), `grad` = ∂H / ∂V
and `γ` (the pdf posteriors), both B × P × N like `pdfposteriors`' γ, and ttl = log Z.  With `grad = false` only the forward kernel
runs (value and ttl, for confidence scoring) and `grad`, `γ` come back as `nothing`.
"""
function pathentropy(b::ROCBatch, V::ROCArray{Float32,3}, lens = nothing; grad = true)
    P, N, B = size(V)
    P == b.P || throw(DimensionMismatch("V has $P pdfs, the FSMs $(b.P)"))
    H = ROCArray{Float32}(undef, B)
    g = grad ? ROCArray{Float32}(undef, B, P, N) : nothing
    γ = grad ? ROCArray{Float32}(undef, B, P, N) : nothing
    ttl = ROCArray{Float32}(undef, B)
    lp = lens === nothing ? Ptr{Int32}(C_NULL) : Ptr{Int32}(pointer(lens))
    check(ccall((:mm_pathentropy_f32, LIB), Cint,
        (Ptr{Cvoid}, Ptr{Float32}, Int64, Int64, Ptr{Int32}, Int64,
         Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Int64, Int64, Int64, Ptr{Float32}, Ptr{Cvoid}),
        b.handle, pointer(V), P * N, P, lp, N,
        pointer(H), grad ? pointer(g) : Ptr{Float32}(C_NULL), grad ? pointer(γ) : Ptr{Float32}(C_NULL), 1, B * P, B, pointer(ttl),
        AMDGPU.stream().stream))
    H, g, γ, ttl
end

"""
    leakyposteriors(b::ROCBatch, V::ROCArray{Float32,3}, lens = nothing; leak = 1f-5) -> (γ, ttl)

Pdf posteriors of the leaky HMM (mm_leakyposteriors_f32 in the header) of a log-semiring batch: `pdfposteriors` with T̂ replaced by
(I + leak · u πᵀ) · T̂ -- after any frame, from any real state, a path may jump with weight leak · π(k) to initial state k.  The
denominator forward-backward of LF-MMI training on chunks.  `V` and `lens` as for `pdfposteriors`; γ is B × P × N, ttl = log Z.
"""
function leakyposteriors(b::ROCBatch, V::ROCArray{Float32,3}, lens = nothing; leak = 1f-5)
    P, N, B = size(V)
    P == b.P || throw(DimensionMismatch("V has $P pdfs, the FSMs $(b.P)"))
    γ = ROCArray{Float32}(undef, B, P, N)
    ttl = ROCArray{Float32}(undef, B)
    lp = lens === nothing ? Ptr{Int32}(C_NULL) : Ptr{Int32}(pointer(lens))
    check(ccall((:mm_leakyposteriors_f32, LIB), Cint,
        (Ptr{Cvoid}, Ptr{Float32}, Int64, Int64, Ptr{Int32}, Int64, Cfloat,
         Ptr{Float32}, Int64, Int64, Int64, Ptr{Float32}, Ptr{Cvoid}),
        b.handle, pointer(V), P * N, P, lp, N, Float32(leak),
        pointer(γ), 1, B * P, B, pointer(ttl),
        AMDGPU.stream().stream))
    γ, ttl
end

"""
    filterposteriors(b::ROCBatch, V::ROCArray{Float32,3}, lens = nothing; state = nothing, filt = true) -> (filt, incr, ttl, state_out)

Forward filtering posteriors with a carried state (mm_filterposteriors_f32 in the header) of a log-semiring batch: `filt` (B × P × N
like `pdfposteriors`' γ) = P(pdf_n = p | V up to frame n), `incr` (N × B) = log P(V_n | V before n), ttl = log Z when `state` is
`nothing`, and `state_out` (`total_states(b)` natural logs: the one-step prediction behind the last frame, the final entries the log
of the alive mass the final weights accept).  `state` = an earlier call's `state_out` continues where that call stopped: chunking is
exact, and log Z = the sum of all `incr` + the last `state_out`'s final entry.  `filt = false` skips the per-pdf pass (`filt` comes
back as `nothing`; the other results keep their bits).  `V` and `lens` as for `pdfposteriors`; `lens[b] = 0` passes the state through.
"""
function filterposteriors(b::ROCBatch, V::ROCArray{Float32,3}, lens = nothing; state = nothing, filt = true)
    P, N, B = size(V)
    P == b.P || throw(DimensionMismatch("V has $P pdfs, the FSMs $(b.P)"))
    S = Int(ccall((:mm_batch_total_states, LIB), Int64, (Ptr{Cvoid},), b.handle))
    state === nothing || length(state) == S || throw(DimensionMismatch("state has $(length(state)) entries, the batch $S states"))
    f = filt ? ROCArray{Float32}(undef, B, P, N) : nothing
    incr = ROCArray{Float32}(undef, N, B)
    ttl = ROCArray{Float32}(undef, B)
    state_out = ROCArray{Float32}(undef, S)
    lp = lens === nothing ? Ptr{Int32}(C_NULL) : Ptr{Int32}(pointer(lens))
    check(ccall((:mm_filterposteriors_f32, LIB), Cint,
        (Ptr{Cvoid}, Ptr{Float32}, Int64, Int64, Ptr{Int32}, Int64, Ptr{Float32}, Ptr{Float32},
         Ptr{Float32}, Int64, Int64, Int64, Ptr{Float32}, Int64, Ptr{Float32}, Ptr{Cvoid}),
        b.handle, pointer(V), P * N, P, lp, N,
        state === nothing ? Ptr{Float32}(C_NULL) : pointer(state), pointer(state_out),
        filt ? pointer(f) : Ptr{Float32}(C_NULL), 1, B * P, B, pointer(incr), N, pointer(ttl),
        AMDGPU.stream().stream))
    f, incr, ttl, state_out
end

"""
    windowposteriors(b::ROCBatch, V::ROCArray{Float32,3}, lens = nothing; state = nothing, closed = nothing, commit = nothing) -> (γ, ttl, lcommit, state_out)

Fixed-lag smoothing posteriors (mm_windowposteriors_f32 in the header) of a log-semiring batch: the forward-backward over a window of
the audio that starts from `state` (an earlier call's `state_out`; `nothing`: the FSMs' own initial vectors) and ends open -- β = 1 on
every real state, the audio goes on -- or, for the utterances with `closed[b] != 0`, on the final weights.  `γ` (B × P × N like
`pdfposteriors`' γ), ttl = log P(window | start), `state_out` = `filterposteriors`' state after `commit[b]` frames (`nothing`: all
`lens[b]`) and `lcommit` the log-likelihood of those frames.  A second window over the frames from `commit` on, from `state_out`,
has this window's γ there and ttl - lcommit as its ttl.  `closed` and `commit` are `ROCVector{Int32}` of length B.
"""
function windowposteriors(b::ROCBatch, V::ROCArray{Float32,3}, lens = nothing; state = nothing, closed = nothing, commit = nothing)
    P, N, B = size(V)
    P == b.P || throw(DimensionMismatch("V has $P pdfs, the FSMs $(b.P)"))
    S = Int(ccall((:mm_batch_total_states, LIB), Int64, (Ptr{Cvoid},), b.handle))
    state === nothing || length(state) == S || throw(DimensionMismatch("state has $(length(state)) entries, the batch $S states"))
    γ = ROCArray{Float32}(undef, B, P, N)
    ttl = ROCArray{Float32}(undef, B)
    lcommit = ROCArray{Float32}(undef, B)
    state_out = ROCArray{Float32}(undef, S)
    ip(x) = x === nothing ? Ptr{Int32}(C_NULL) : Ptr{Int32}(pointer(x))
    check(ccall((:mm_windowposteriors_f32, LIB), Cint,
        (Ptr{Cvoid}, Ptr{Float32}, Int64, Int64, Ptr{Int32}, Int64, Ptr{Float32}, Ptr{Int32}, Ptr{Int32},
         Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Int64, Int64, Int64, Ptr{Float32}, Ptr{Cvoid}),
        b.handle, pointer(V), P * N, P, ip(lens), N,
        state === nothing ? Ptr{Float32}(C_NULL) : pointer(state), ip(closed), ip(commit),
        pointer(state_out), pointer(lcommit), pointer(γ), 1, B * P, B, pointer(ttl),
        AMDGPU.stream().stream))
    γ, ttl, lcommit, state_out
end

"""
    segmentposteriors(b::ROCBatch, V::ROCArray{Float32,3}, lens = nothing; state = nothing, end_mode = nothing, end_in = nothing) -> (γ, ttl, lend, end_out)

Segment posteriors (mm_segmentposteriors_f32 in the header) of a log-semiring batch: the forward-backward over a segment of the audio
that starts from `state` like a window and ends open (`end_mode[b] == 0`, or `end_mode === nothing`), on the carried end vector
`end_in` (`end_mode[b] == 2`; the layout of `state`, natural log) or on the final weights (anything else).  `γ` (B × P × N), ttl =
log Σ a_len b_len, and what the segment BEFORE this one ends on: `end_out` = log b₀ - `lend`, `lend` = log max b₀.  Chaining is
exact: the exact smoothing posteriors of a long recording are `filterposteriors` over the chunks, which saves each chunk's start
state, then this call over the chunks in reverse, each on the `end_out` of the chunk behind it -- in the workspace of one chunk.
`end_mode` is a `ROCVector{Int32}` of length B.
"""
function segmentposteriors(b::ROCBatch, V::ROCArray{Float32,3}, lens = nothing; state = nothing, end_mode = nothing, end_in = nothing)
    P, N, B = size(V)
    P == b.P || throw(DimensionMismatch("V has $P pdfs, the FSMs $(b.P)"))
    S = Int(ccall((:mm_batch_total_states, LIB), Int64, (Ptr{Cvoid},), b.handle))
    state === nothing || length(state) == S || throw(DimensionMismatch("state has $(length(state)) entries, the batch $S states"))
    end_in === nothing || length(end_in) == S || throw(DimensionMismatch("end_in has $(length(end_in)) entries, the batch $S states"))
    γ = ROCArray{Float32}(undef, B, P, N)
    ttl = ROCArray{Float32}(undef, B)
    lend = ROCArray{Float32}(undef, B)
    end_out = ROCArray{Float32}(undef, S)
    ip(x) = x === nothing ? Ptr{Int32}(C_NULL) : Ptr{Int32}(pointer(x))
    fp(x) = x === nothing ? Ptr{Float32}(C_NULL) : pointer(x)
    check(ccall((:mm_segmentposteriors_f32, LIB), Cint,
        (Ptr{Cvoid}, Ptr{Float32}, Int64, Int64, Ptr{Int32}, Int64, Ptr{Float32}, Ptr{Int32}, Ptr{Float32},
         Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Int64, Int64, Int64, Ptr{Float32}, Ptr{Cvoid}),
        b.handle, pointer(V), P * N, P, ip(lens), N,
        fp(state), ip(end_mode), fp(end_in),
        pointer(end_out), pointer(lend), pointer(γ), 1, B * P, B, pointer(ttl),
        AMDGPU.stream().stream))
    γ, ttl, lend, end_out
end

"""
    pdfposteriors(fsm::FSM{K}, V̂s::Vector{<:ROCMatrix}, Ĉs; expanded = true, seqlengths = nothing) -> (γ, ttl)

The reference's own signature (src/inference.jl:145): `fsm` the `rawunion` of the batch's FSMs (src/fsmops.jl:28-36), `V̂s`
one (P+1) × (N+1) matrix per utterance as `expand` made them, `Ĉs` the state maps -- examples/test_cuda.jl:128 runs
unchanged but for the array type.  The blocks of the union are cut apart again by the rows of the `Ĉs` (block b has
size(Ĉs[b], 1) states) and looked up in a PROCESS-WIDE cache of compiled graphs keyed by their content (`hash` of the
block's T̂, α̂ and Ĉ): a graph is packed and uploaded the first time it is seen -- the misses of one call together, by
`compile_many` -- and found again on every later call (the denominator graph; an utterance's numerator across epochs).
The whole batch is remembered per `(fsm, Ĉs)` object pair as well, so a loop that passes the same objects pays one
dictionary look-up.  `V̂s` are stacked on the device like `vcat(V̂s...)` (:146).
With Float32 log-semiring (or, since round 6, ProbSemiring) FSMs, one-hot `Ĉs` and `expanded = true` the fast kernels run on
V̂[1:P, 1:N, b] IN PLACE (strides).
The lengths: `seqlengths` (what `expand` was given: a Vector or ROCVector of integers) keeps the call asynchronous; without it
they are read off the phony row on the host, and the form `expand` gives a matrix (phony row zero(K) up to the length and
one(K) after, real rows zero(K) beyond it) is CHECKED -- a matrix of another form goes to the generic entry like
`expanded = false`.  Anything else (Float64; other semirings; general sparse `Ĉs`) goes to `pdfposteriors_generic`.
Nothing synchronises the device: the batch lives in the cache, and the stacked V̂ and the lengths stay referenced by the batch
(`b.keep`) until the next call on it replaces them -- stream order then guarantees the earlier call has read them.
"""
function pdfposteriors(fsm::FSM{K}, V̂s::Vector{<:ROCMatrix{T}}, Ĉs::Vector{<:AbstractSparseMatrix}; expanded::Bool = true,
                       seqlengths = nothing) where {K, T}
    B = length(V̂s)
    B == length(Ĉs) || throw(DimensionMismatch("one Ĉ per utterance"))
    P1, N1 = size(V̂s[1])
    all(size(v) == (P1, N1) for v in V̂s) || throw(DimensionMismatch("all V̂ must share one (P+1) × (N+1) shape"))
    all(size(Ĉ, 2) == P1 for Ĉ in Ĉs) || throw(DimensionMismatch("V̂ has $P1 rows, a Ĉ has another number of pdfs"))
    b, onehot = _cached_batch(fsm, Ĉs)
    V̂ = cat(V̂s...; dims = 3)                                    # (P+1) × (N+1) × B on the device
    # (ProbSemiring{Float32} too: the library keeps a log-semiring twin of such FSMs and runs the fast kernels on log V̂ -- V̂ then
    # holds likelihoods, ttl comes back as a probability: mm_pdfposteriors_f32 in the header)
    fast = expanded && onehot && (K <: LogSemiring || K <: ProbSemiring) && T === Float32 && eltype(val(one(K))) === Float32
    z0, o1 = K <: ProbSemiring ? (0f0, 1f0) : (-Inf32, 0f0)      # val(zero(K)), val(one(K))
    P, N = P1 - 1, N1 - 1
    lens = nothing
    if fast
        if seqlengths !== nothing
            lens = seqlengths isa ROCArray ? ROCArray{Int32}(seqlengths) : ROCArray(Int32.(collect(seqlengths)))
        else
            # expand (src/inference.jl:54-60): the phony row is zero(K) up to seqlength and one(K) after, the real rows are
            # zero(K) beyond it -- read and verified on the host (one round trip; pass `seqlengths` to avoid it)
            ph = Array(V̂[P1, :, :])                             # (N+1) × B
            L = vec(sum(ph .== z0, dims = 1))
            step_ok = all(all(ph[1:L[j], j] .== z0) && all(ph[L[j]+1:end, j] .== o1) && L[j] <= N for j in 1:B)
            tail_ok = step_ok && all(mapreduce(x -> x == z0, &, V̂[1:P, L[j]+1:N1, j]; init = true) for j in 1:B if L[j] < N1)   # (a GPU reduction returns a host scalar)
            fast = step_ok && tail_ok
            lens = ROCArray(Int32.(L))
        end
    end
    fast || return pdfposteriors_generic(b, V̂, onehot ? nothing : Ĉs)
    γ = ROCArray{Float32}(undef, B, P, N)
    ttl = ROCArray{Float32}(undef, B)
    # V̂ (b, n, p) -> p + P1*n + P1*N1*b: the kernels read the real pdfs and frames in place
    check(ccall((:mm_pdfposteriors_f32, LIB), Cint,
        (Ptr{Cvoid}, Ptr{Float32}, Int64, Int64, Ptr{Int32}, Int64, Ptr{Float32}, Int64, Int64, Int64,
         Ptr{Float32}, Ptr{Cvoid}),
        b.handle, pointer(V̂), P1 * N1, P1, pointer(lens), N, pointer(γ), 1, B * P, B, pointer(ttl),
        AMDGPU.stream().stream))
    # (asynchronous: the batch lives in the cache; the stacked V̂ and the lengths are kept until the NEXT call on this batch
    # replaces them -- stream order then guarantees this call has read them)
    b.keep = (V̂, lens)
    γ, ttl
end

# ---- the compiled-graph cache behind the method above: two BOUNDED least-recently-used tables
# _COMPILED: 128-bit content key of (T̂ block, α̂ block, Ĉ) -> ROCCompiledFSM (two independent 64-bit hashes of the same fields: a
#            collision of both is not a practical event; the Python mirror uses a 128-bit digest likewise)
# _BATCHES:  identity of the caller's fsm object -> (Ĉs object, ROCBatch, onehot): a loop that passes the same objects pays one look-up.
# Both hold strong references, so both are bounded: a training loop that builds a new numerator union every step would otherwise
# keep every ROCBatch (its device workspace, its descriptors, its last stacked V̂ through `keep`) until the device is full.  A batch
# that falls out of _BATCHES is destroyed at once (mm_batch_destroy frees with hipFree, which waits for the device: a call still in
# flight on it finishes first); compiled graphs that fall out of _COMPILED are freed by their finalizers when no batch uses them.
mutable struct _LRU{Kt, Vt}
    d::Dict{Kt, Tuple{Vt, Int}}       # key -> (value, stamp of its last use)
    clock::Int
    limit::Int
end
_LRU{Kt, Vt}(limit::Integer) where {Kt, Vt} = _LRU{Kt, Vt}(Dict{Kt, Tuple{Vt, Int}}(), 0, Int(limit))
function _lru_get(c::_LRU, k)
    e = get(c.d, k, nothing)
    e === nothing && return nothing
    c.clock += 1
    c.d[k] = (e[1], c.clock)
    e[1]
end
"Insert; returns the values that fell out (oldest first) so that the caller can release what they own."
function _lru_put!(c::_LRU{Kt, Vt}, k, v) where {Kt, Vt}
    c.clock += 1
    c.d[k] = (v, c.clock)
    out = Vt[]
    while length(c.d) > c.limit
        oldest = first(c.d)
        for kv in c.d
            kv.second[2] < oldest.second[2] && (oldest = kv)
        end
        push!(out, oldest.second[1])
        delete!(c.d, oldest.first)
    end
    out
end
const _COMPILED = _LRU{NTuple{2, UInt64}, Any}(8192)
const _BATCHES = _LRU{UInt, Any}(16)
"Forget every compiled graph and batch the reference-shaped `pdfposteriors` has cached."
function compiled_cache_clear!()
    for e in values(_BATCHES.d)
        finalize(e[1][2])
    end
    empty!(_BATCHES.d); empty!(_COMPILED.d); nothing
end
"Bounds of the two tables: compiled graphs (default 8192) and whole batches (default 16)."
compiled_cache_limits!(; graphs::Integer = 8192, batches::Integer = 16) = (_COMPILED.limit = graphs; _BATCHES.limit = batches; nothing)

_isonehot(Ĉ::AbstractSparseMatrix{K}) where K =
    all(diff(SparseMatrixCSC(copy(Ĉ')).colptr) .== 1) && all(x -> x == one(K), nonzeros(Ĉ))   # (one(ProbSemiring) = 1: not iszero ∘ val)

function _cached_batch(fsm::FSM{K}, Ĉs) where K
    id = objectid(fsm)
    hit = _lru_get(_BATCHES, id)
    # (objectid of an immutable FSM is the identity of its fields: the same T̂ / α̂ / λ arrays; the entry keeps `fsm` itself, so the id
    # cannot be reused by another object while the entry lives)
    hit !== nothing && hit[4] === fsm && hit[1] === Ĉs && return hit[2], hit[3]
    T̂, α̂ = SparseMatrixCSC(fsm.T̂), SparseVector(fsm.α̂)
    sum(size(Ĉ, 1) for Ĉ in Ĉs) == size(T̂, 1) || throw(DimensionMismatch("the Ĉs' rows do not add up to the states of fsm"))
    onehot = all(_isonehot, Ĉs)
    keys = NTuple{2, UInt64}[]
    blocks = Dict{NTuple{2, UInt64}, Any}()
    lo = 0
    for Ĉ in Ĉs
        r = lo+1:lo+size(Ĉ, 1)
        Tb, ab = T̂[r, r], α̂[r]
        # (a general sparse Ĉ rides along as an argument of the generic entry: its FSM handle gets a placeholder map)
        Cb = onehot ? Ĉ : sparse(1:size(Ĉ, 1), [fill(1, size(Ĉ, 1) - 1); size(Ĉ, 2)], fill(one(K), size(Ĉ, 1)), size(Ĉ, 1), size(Ĉ, 2))
        content = (K, Tb.colptr, Tb.rowval, val.(nonzeros(Tb)), SparseArrays.nonzeroinds(ab), val.(nonzeros(ab)), Cb.colptr, Cb.rowval, size(Cb))
        k = (hash(content, UInt(0x243f6a8885a308d3)), hash(content, UInt(0x13198a2e03707344)))
        push!(keys, k)
        haskey(_COMPILED.d, k) || haskey(blocks, k) || (blocks[k] = (Tb, ab, Cb))
        lo = last(r)
    end
    if !isempty(blocks)                      # the misses of this call, compiled together
        ks = collect(Base.keys(blocks))
        if length(ks) == 1
            Tb, ab, Cb = blocks[ks[1]]
            _lru_put!(_COMPILED, ks[1], _create(K, Tb, ab, Cb))
        else
            fs = [FSM(blocks[k][2], blocks[k][1], eltype(fsm.λ)[]) for k in ks]   # (the struct's own constructor, src/fsm.jl:7-17, 44: labels play no part in inference)
            made = compile_many(fs, [blocks[k][3] for k in ks])
            for (k, c) in zip(ks, made)
                _lru_put!(_COMPILED, k, c)
            end
        end
    end
    # (the graphs of THIS call are fetched before anything else is inserted: a batch larger than the table's bound still finds them)
    cfs = ROCCompiledFSM{K}[]
    for k in keys
        c = _lru_get(_COMPILED, k)
        c === nothing && error("compiled-graph cache: the bound ($(_COMPILED.limit)) is smaller than one batch's distinct graphs")
        push!(cfs, c::ROCCompiledFSM{K})
    end
    b = batch(cfs...)
    for old in _lru_put!(_BATCHES, id, (Ĉs, b, onehot, fsm))
        finalize(old[2])                      # mm_batch_destroy now: workspace, descriptors, and the V̂ it kept
    end
    b, onehot
end

function _recursion(sym::Symbol, b::ROCBatch, V::ROCArray{Float32,3}, lens)
    P, N, B = size(V)
    total = ccall((:mm_batch_total_states, LIB), Int64, (Ptr{Cvoid},), b.handle)
    out = ROCArray{Float32}(undef, total, N + 1)          # (ΣS1) × (N+1) like state_A / state_B
    lp = lens === nothing ? Ptr{Int32}(C_NULL) : Ptr{Int32}(pointer(lens))
    check(ccall((sym, LIB), Cint,
        (Ptr{Cvoid}, Ptr{Float32}, Int64, Int64, Ptr{Int32}, Int64, Ptr{Float32}, Int64, Ptr{Cvoid}),
        b.handle, pointer(V), P * N, P, lp, N, pointer(out), total, AMDGPU.stream().stream))
    out
end

"αrecursion(α̂, T̂ᵀ, ĈV̂) (src/inference.jl:62-74) as pdfposteriors calls it (:150-152)."
αrecursion(b::ROCBatch, V::ROCArray{Float32,3}, lens = nothing) =
    _recursion(:mm_alpharecursion_f32, b, V, lens)
"βrecursion(T̂, ĈV̂) (src/inference.jl:99-110)."
βrecursion(b::ROCBatch, V::ROCArray{Float32,3}, lens = nothing) =
    _recursion(:mm_betarecursion_f32, b, V, lens)

"""
    bestpath(b::ROCBatch{<:TropicalSemiring}, V, lens) -> (paths, scores)

docs/src/inference.md:6 (absent from src/ at v0.10.0).  States are returned 1-based.
"""
function bestpath(b::ROCBatch{K}, V::ROCArray{Float32,3}, lens = nothing) where K <: TropicalSemiring
    P, N, B = size(V)
    path = ROCArray{Int32}(undef, N, B)
    score = ROCArray{Float32}(undef, B)
    lp = lens === nothing ? Ptr{Int32}(C_NULL) : Ptr{Int32}(pointer(lens))
    check(ccall((:mm_viterbi_f32, LIB), Cint,
        (Ptr{Cvoid}, Ptr{Float32}, Int64, Int64, Ptr{Int32}, Int64, Ptr{Int32}, Int64, Ptr{Float32},
         Ptr{Int32}, Int64, Ptr{Cvoid}),
        b.handle, pointer(V), P * N, P, lp, N, pointer(path), N, pointer(score), C_NULL, 0,
        AMDGPU.stream().stream))
    Array(path) .+ Int32(1), Array(score)
end

"""
    viterbiwindow(b::ROCBatch{<:TropicalSemiring}, V, lens = nothing; state = nothing, closed = nothing, commit = nothing, commit_converged = false)
        -> (paths, scores, converged, ncommit, mcommit, state_out)

Windowed best paths (mm_viterbiwindow_f32 in the header): the Viterbi recursion over a window of the audio that starts from `state`
(an earlier call's `state_out`; `nothing`: the FSMs' own initial vectors) and ends open -- on the best real state, the audio goes
on -- or, for the utterances with `closed[b] != 0`, in the final state.  `converged[b]` is the last frame every surviving path
passes: the path up to it is final.  `state_out` and `mcommit` belong to frame `commit[b]` (with `commit_converged`: no earlier than
`converged[b]`), `ncommit` says which; a second window over the frames behind it, from `state_out`, continues the path.  States are
returned 1-based (0: no state), `closed` and `commit` are `ROCVector{Int32}` of length B.
"""
function viterbiwindow(b::ROCBatch{K}, V::ROCArray{Float32,3}, lens = nothing; state = nothing, closed = nothing, commit = nothing,
                       commit_converged::Bool = false) where K <: TropicalSemiring
    P, N, B = size(V)
    S = Int(ccall((:mm_batch_total_states, LIB), Int64, (Ptr{Cvoid},), b.handle))
    state === nothing || length(state) == S || throw(DimensionMismatch("state has $(length(state)) entries, the batch $S states"))
    path = ROCArray{Int32}(undef, N, B)
    score = ROCArray{Float32}(undef, B)
    converged = ROCArray{Int32}(undef, B)
    ncommit = ROCArray{Int32}(undef, B)
    mcommit = ROCArray{Float32}(undef, B)
    state_out = ROCArray{Float32}(undef, S)
    ip(x) = x === nothing ? Ptr{Int32}(C_NULL) : Ptr{Int32}(pointer(x))
    check(ccall((:mm_viterbiwindow_f32, LIB), Cint,
        (Ptr{Cvoid}, Ptr{Float32}, Int64, Int64, Ptr{Int32}, Int64, Ptr{Float32}, Ptr{Int32}, Ptr{Int32}, Cint,
         Ptr{Float32}, Ptr{Float32}, Ptr{Int32}, Ptr{Int32}, Int64, Ptr{Float32}, Ptr{Int32}, Ptr{Cvoid}),
        b.handle, pointer(V), P * N, P, ip(lens), N,
        state === nothing ? Ptr{Float32}(C_NULL) : pointer(state), ip(closed), ip(commit), commit_converged ? 1 : 0,
        pointer(state_out), pointer(mcommit), pointer(ncommit), pointer(path), N, pointer(score), pointer(converged),
        AMDGPU.stream().stream))
    Array(path) .+ Int32(1), Array(score), Array(converged), Array(ncommit), Array(mcommit), state_out
end

"""
    set_path_classes!(b::ROCBatch{<:TropicalSemiring}, classes, C = nothing) -> C

The class of every stored entry of `T̂` for `classpath` (mm_batch_set_path_classes in the header): the arguments of
`set_arc_classes!`, on a tropical batch; at most 65534 classes.  Host work only; calling it again replaces the plan.
"""
function set_path_classes!(b::ROCBatch{K}, classes::AbstractVector, C = nothing) where K <: TropicalSemiring
    shared = !(eltype(classes) <: AbstractVector)
    parts = shared ? [classes] : classes
    flat = Int32[]
    offs = Int64[0]
    for c in parts
        append!(flat, Int32.(c))
        push!(offs, length(flat))
    end
    nc = C === nothing ? max(1, Int(maximum(flat; init = Int32(0))) + 1) : Int(C)
    op = shared ? Ptr{Int64}(C_NULL) : pointer(offs)
    GC.@preserve flat offs check(ccall((:mm_batch_set_path_classes, LIB), Cint, (Ptr{Cvoid}, Ptr{Int32}, Ptr{Int64}, Int32),
        b.handle, pointer(flat), op, Int32(nc)))
    nc
end

"(C, cap) of the batch's path-class plan (mm_batch_path_class_info): the classes of the plan (0: none), the most classes whose score rows `classpath` takes"
function path_class_info(b::ROCBatch)
    c, cap = Ref{Int32}(0), Ref{Int64}(0)
    check(ccall((:mm_batch_path_class_info, LIB), Cint, (Ptr{Cvoid}, Ptr{Int32}, Ptr{Int64}), b.handle, c, cap))
    (C = Int(c[]), cap = cap[])
end

"""
    classpath(b::ROCBatch{<:TropicalSemiring}, V, U = nothing, lens = nothing) -> (paths, classes, scores)

Best paths that report arc classes, under per-frame arc-class scores (mm_classpath_f32 in the header): under the classes of
`set_path_classes!` the entry taken between frames t and t + 1 adds `U[c, t, u]` to its own weight (`U` a `C × N × B`
`ROCArray{Float32,3}`, finite or `-Inf`; `nothing`: no scores -- paths and scores are then `bestpath`'s).  States are returned
1-based (0: no state); `classes[t, u]` is the 0-based class of the entry taken at transition t, -1 for an unclassified entry,
beyond the length and without a path.
"""
function classpath(b::ROCBatch{K}, V::ROCArray{Float32,3}, U = nothing, lens = nothing) where K <: TropicalSemiring
    P, N, B = size(V)
    nc = max(1, path_class_info(b).C)
    U === nothing || size(U) == (nc, N, B) || throw(DimensionMismatch("U must be $nc × $N × $B"))
    path = ROCArray{Int32}(undef, N, B)
    classes = ROCArray{Int32}(undef, N, B)
    score = ROCArray{Float32}(undef, B)
    lp = lens === nothing ? Ptr{Int32}(C_NULL) : Ptr{Int32}(pointer(lens))
    up = U === nothing ? Ptr{Float32}(C_NULL) : Ptr{Float32}(pointer(U))
    check(ccall((:mm_classpath_f32, LIB), Cint,
        (Ptr{Cvoid}, Ptr{Float32}, Int64, Int64, Ptr{Int32}, Int64, Ptr{Float32}, Int64, Int64, Int64, Ptr{Int32}, Int64, Ptr{Int32}, Int64,
         Ptr{Float32}, Ptr{Cvoid}),
        b.handle, pointer(V), P * N, P, lp, N, up, nc * N, nc, 1, pointer(path), N, pointer(classes), N, pointer(score),
        AMDGPU.stream().stream))
    Array(path) .+ Int32(1), Array(classes), Array(score)
end

"""
    maxstateposteriors(b::ROCBatch{<:TropicalSemiring}, V, lens) -> Matrix{Float32}

docs/src/inference.md:5 (absent from src/ at v0.10.0): the max-marginals alpha (*) beta (/) best of the tropical
semiring, (sum of S+1) x (N+1), 0 along a best path.
"""
maxstateposteriors(b::ROCBatch{K}, V::ROCArray{Float32,3}, lens = nothing) where K <: TropicalSemiring =
    _recursion(:mm_maxstateposteriors_f32, b, V, lens)   # one device call: tropical alpha, beta and the combination

"""
    lattice(b::ROCBatch{<:TropicalSemiring}, V, beam, lens = nothing) -> (counts, offsets, arc, score, best)

Beam-pruned best-path lattices (mm_lattice_f32 in the header): for every utterance u and transition t the stored entries of `T̂`
(1-based here, ascending, in `arcposteriors`' entry order) on a complete path within `beam[u]` of the best path, with their
through-scores relative to it.  `beam` is a number or a vector of B, natural log.  `counts` is `N × B`; `offsets` (length
`N·B + 1`, 0-based record numbers) is their exclusive prefix sum in (u, t) order: the records of (u, t) are
`offsets[(u-1)N + t] + 1 : offsets[(u-1)N + t + 1]`.  Two calls: the count-only one, whose total is read back (one
synchronisation), then the full one.
"""
function lattice(b::ROCBatch{K}, V::ROCArray{Float32,3}, beam, lens = nothing) where K <: TropicalSemiring
    P, N, B = size(V)
    bm = ROCArray(beam isa Number ? fill(Float32(beam), B) : Float32.(collect(beam)))
    length(bm) == B || throw(DimensionMismatch("beam must be a number or a vector of $B"))
    counts = ROCArray{Int32}(undef, N, B)
    total = ROCArray{Int64}(undef, 1)
    best = ROCArray{Float32}(undef, B)
    lp = lens === nothing ? Ptr{Int32}(C_NULL) : Ptr{Int32}(pointer(lens))
    check(ccall((:mm_lattice_f32, LIB), Cint,
        (Ptr{Cvoid}, Ptr{Float32}, Int64, Int64, Ptr{Int32}, Int64, Ptr{Float32}, Ptr{Int32}, Int64, Ptr{Int64}, Ptr{Float32}, Ptr{Int32},
         Ptr{Float32}, Int64, Ptr{Cvoid}),
        b.handle, pointer(V), P * N, P, lp, N, pointer(bm), pointer(counts), N, pointer(total), pointer(best), Ptr{Int32}(C_NULL),
        Ptr{Float32}(C_NULL), 0, AMDGPU.stream().stream))
    n = Array(total)[1]
    arc = ROCArray{Int32}(undef, n)
    score = ROCArray{Float32}(undef, n)
    check(ccall((:mm_lattice_f32, LIB), Cint,
        (Ptr{Cvoid}, Ptr{Float32}, Int64, Int64, Ptr{Int32}, Int64, Ptr{Float32}, Ptr{Int32}, Int64, Ptr{Int64}, Ptr{Float32}, Ptr{Int32},
         Ptr{Float32}, Int64, Ptr{Cvoid}),
        b.handle, pointer(V), P * N, P, lp, N, pointer(bm), pointer(counts), N, pointer(total), pointer(best), pointer(arc),
        pointer(score), n, AMDGPU.stream().stream))
    c = Array(counts)
    c, vcat(Int64(0), cumsum(Int64.(vec(c)))), Array(arc) .+ Int32(1), Array(score), Array(best)
end

"""
    latticeposteriors(b::ROCBatch{<:TropicalSemiring}, V, offsets, arc, lens = nothing; extra = nothing, want_gamma = true)
        -> (post, logz, gamma)

Lattice posteriors (mm_latticeposteriors_f32 in the header): the log-semiring forward-backward over the records of a lattice --
`offsets` and `arc` as `lattice` returns them (`arc` 1-based), or a subset that keeps the order within a transition -- under the
emissions `V` of this call and an optional score `extra` per record.  `post[r]` is the log posterior of record r, `logz` (B) the
log-sum of the lattice's paths, `gamma` (`P × N × B`, `nothing` without `want_gamma`) the pdf occupancies: the gradient of `logz`
against `V`; `exp.(post)` is the gradient against `extra`.  `lens` are those of the lattice call.
"""
function latticeposteriors(b::ROCBatch{K}, V::ROCArray{Float32,3}, offsets::AbstractVector{<:Integer}, arc::AbstractVector{<:Integer},
                           lens = nothing; extra = nothing, want_gamma::Bool = true) where K <: TropicalSemiring
    P, N, B = size(V)
    length(offsets) == N * B + 1 || throw(DimensionMismatch("offsets must have N·B + 1 = $(N * B + 1) entries"))
    n = length(arc)
    offsets[end] <= n || throw(ArgumentError("the lattice has $(offsets[end]) records, arc holds $n"))
    extra === nothing || length(extra) == n || throw(DimensionMismatch("extra must hold one score per record ($n)"))
    offs = ROCArray(Int64.(collect(offsets)))
    arcd = ROCArray(Int32.(collect(arc)) .- Int32(1))
    ex = extra === nothing ? nothing : ROCArray(Float32.(collect(extra)))
    post = ROCArray{Float32}(undef, n)
    logz = ROCArray{Float32}(undef, B)
    gamma = want_gamma ? ROCArray{Float32}(undef, P, N, B) : nothing
    lp = lens === nothing ? Ptr{Int32}(C_NULL) : Ptr{Int32}(pointer(lens))
    check(ccall((:mm_latticeposteriors_f32, LIB), Cint,
        (Ptr{Cvoid}, Ptr{Float32}, Int64, Int64, Ptr{Int32}, Int64, Ptr{Int64}, Ptr{Int32}, Int64, Ptr{Float32}, Ptr{Float32}, Ptr{Float32},
         Ptr{Float32}, Int64, Int64, Ptr{Cvoid}),
        b.handle, pointer(V), P * N, P, lp, N, pointer(offs), pointer(arcd), n, ex === nothing ? Ptr{Float32}(C_NULL) : pointer(ex),
        pointer(post), pointer(logz), gamma === nothing ? Ptr{Float32}(C_NULL) : pointer(gamma), P * N, P, AMDGPU.stream().stream))
    Array(post), Array(logz), gamma === nothing ? nothing : Array(gamma)
end

"""
    latticecost(b::ROCBatch{<:TropicalSemiring}, V, offsets, arc, cost, lens = nothing; extra = nothing, want_grad = true,
                want_gamma = false) -> (risk, diff, post, logz, grad, gamma)

Lattice expected cost (mm_latticecost_f32 in the header): the expectation of the summed `cost` of a path's records over the paths of
a lattice, weighed as `latticeposteriors` weighs them, and its gradient (lattice-based sMBR / MPE).  `risk` (B), `diff[r]` the
gradient against `extra`, `post` and `logz` those of `latticeposteriors`, `grad` (`P × N × B`) the gradient against `V`, `gamma` the
pdf occupancies (`nothing` when not asked for); `exp.(post)` is the gradient against `cost`.
"""
function latticecost(b::ROCBatch{K}, V::ROCArray{Float32,3}, offsets::AbstractVector{<:Integer}, arc::AbstractVector{<:Integer},
                     cost::AbstractVector{<:Real}, lens = nothing; extra = nothing, want_grad::Bool = true,
                     want_gamma::Bool = false) where K <: TropicalSemiring
    P, N, B = size(V)
    length(offsets) == N * B + 1 || throw(DimensionMismatch("offsets must have N·B + 1 = $(N * B + 1) entries"))
    n = length(arc)
    offsets[end] <= n || throw(ArgumentError("the lattice has $(offsets[end]) records, arc holds $n"))
    length(cost) == n || throw(DimensionMismatch("cost must hold one cost per record ($n)"))
    extra === nothing || length(extra) == n || throw(DimensionMismatch("extra must hold one score per record ($n)"))
    offs = ROCArray(Int64.(collect(offsets)))
    arcd = ROCArray(Int32.(collect(arc)) .- Int32(1))
    cs = ROCArray(Float32.(collect(cost)))
    ex = extra === nothing ? nothing : ROCArray(Float32.(collect(extra)))
    risk = ROCArray{Float32}(undef, B)
    diff = ROCArray{Float32}(undef, n)
    post = ROCArray{Float32}(undef, n)
    logz = ROCArray{Float32}(undef, B)
    grad = want_grad ? ROCArray{Float32}(undef, P, N, B) : nothing
    gamma = want_gamma ? ROCArray{Float32}(undef, P, N, B) : nothing
    lp = lens === nothing ? Ptr{Int32}(C_NULL) : Ptr{Int32}(pointer(lens))
    check(ccall((:mm_latticecost_f32, LIB), Cint,
        (Ptr{Cvoid}, Ptr{Float32}, Int64, Int64, Ptr{Int32}, Int64, Ptr{Int64}, Ptr{Int32}, Int64, Ptr{Float32}, Ptr{Float32}, Ptr{Float32},
         Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Int64, Int64, Ptr{Cvoid}),
        b.handle, pointer(V), P * N, P, lp, N, pointer(offs), pointer(arcd), n, ex === nothing ? Ptr{Float32}(C_NULL) : pointer(ex),
        pointer(cs), pointer(risk), pointer(diff), pointer(post), pointer(logz), grad === nothing ? Ptr{Float32}(C_NULL) : pointer(grad),
        gamma === nothing ? Ptr{Float32}(C_NULL) : pointer(gamma), P * N, P, AMDGPU.stream().stream))
    Array(risk), Array(diff), Array(post), Array(logz), grad === nothing ? nothing : Array(grad), gamma === nothing ? nothing : Array(gamma)
end

"""
    latticebest(b::ROCBatch{<:TropicalSemiring}, V, offsets, arc, lens = nothing; extra = nothing, want_path = true)
        -> (best, score, rec, path)

Lattice best paths (mm_latticebest_f32 in the header), the tropical twin of `latticeposteriors`: `best` (B) the weight of the best
path of the lattice under the emissions `V` of this call and the optional score `extra` per record, `score[r]` the best path through
record r minus `best`, `rec` (`N × B`) the best path's record of every transition (1-based into `arc`, 0: none) and `path` (`N × B`)
the source state of that record (1-based, 0: none); `nothing` for both without `want_path`.
"""
function latticebest(b::ROCBatch{K}, V::ROCArray{Float32,3}, offsets::AbstractVector{<:Integer}, arc::AbstractVector{<:Integer},
                     lens = nothing; extra = nothing, want_path::Bool = true) where K <: TropicalSemiring
    P, N, B = size(V)
    length(offsets) == N * B + 1 || throw(DimensionMismatch("offsets must have N·B + 1 = $(N * B + 1) entries"))
    n = length(arc)
    offsets[end] <= n || throw(ArgumentError("the lattice has $(offsets[end]) records, arc holds $n"))
    extra === nothing || length(extra) == n || throw(DimensionMismatch("extra must hold one score per record ($n)"))
    offs = ROCArray(Int64.(collect(offsets)))
    arcd = ROCArray(Int32.(collect(arc)) .- Int32(1))
    ex = extra === nothing ? nothing : ROCArray(Float32.(collect(extra)))
    best = ROCArray{Float32}(undef, B)
    score = ROCArray{Float32}(undef, n)
    rec = want_path ? ROCArray{Int64}(undef, N, B) : nothing
    path = want_path ? ROCArray{Int32}(undef, N, B) : nothing
    lp = lens === nothing ? Ptr{Int32}(C_NULL) : Ptr{Int32}(pointer(lens))
    check(ccall((:mm_latticebest_f32, LIB), Cint,
        (Ptr{Cvoid}, Ptr{Float32}, Int64, Int64, Ptr{Int32}, Int64, Ptr{Int64}, Ptr{Int32}, Int64, Ptr{Float32}, Ptr{Float32}, Ptr{Float32},
         Ptr{Int64}, Int64, Ptr{Int32}, Int64, Ptr{Cvoid}),
        b.handle, pointer(V), P * N, P, lp, N, pointer(offs), pointer(arcd), n, ex === nothing ? Ptr{Float32}(C_NULL) : pointer(ex),
        pointer(best), pointer(score), rec === nothing ? Ptr{Int64}(C_NULL) : pointer(rec), N,
        path === nothing ? Ptr{Int32}(C_NULL) : pointer(path), N, AMDGPU.stream().stream))
    Array(best), Array(score), rec === nothing ? nothing : Array(rec) .+ Int64(1), path === nothing ? nothing : Array(path) .+ Int32(1)
end

"""
    latticesample(b::ROCBatch{<:TropicalSemiring}, V, offsets, arc, nsamples, lens = nothing; seed = 0, extra = nothing,
                  want_path = true, want_logprob = true) -> (rec, path, logprob, logz)

Lattice path sampling (mm_latticesample_f32 in the header): `nsamples` independent draws per utterance from the posterior over the
record sequences of the lattice under the emissions `V` of this call and the optional score `extra` per record.  `rec`
(`N × nsamples × B`) the samples' records (1-based into `arc`, 0: none), `path` (`N × nsamples × B`) their source states (1-based,
0: none; `nothing` without `want_path`), `logprob` (`nsamples × B`) the log posterior of every sample (`nothing` without
`want_logprob`), `logz` (B) as `latticeposteriors` returns it.  A sample depends on the inputs, `seed`, its utterance's position and
its own index alone.
"""
function latticesample(b::ROCBatch{K}, V::ROCArray{Float32,3}, offsets::AbstractVector{<:Integer}, arc::AbstractVector{<:Integer},
                       nsamples::Integer, lens = nothing; seed::Integer = 0, extra = nothing, want_path::Bool = true,
                       want_logprob::Bool = true) where K <: TropicalSemiring
    P, N, B = size(V)
    nsamples >= 1 || throw(ArgumentError("nsamples must be >= 1"))
    length(offsets) == N * B + 1 || throw(DimensionMismatch("offsets must have N·B + 1 = $(N * B + 1) entries"))
    n = length(arc)
    offsets[end] <= n || throw(ArgumentError("the lattice has $(offsets[end]) records, arc holds $n"))
    extra === nothing || length(extra) == n || throw(DimensionMismatch("extra must hold one score per record ($n)"))
    offs = ROCArray(Int64.(collect(offsets)))
    arcd = ROCArray(Int32.(collect(arc)) .- Int32(1))
    ex = extra === nothing ? nothing : ROCArray(Float32.(collect(extra)))
    fwd = ROCArray{Float32}(undef, n)
    rec = ROCArray{Int64}(undef, N, nsamples, B)
    path = want_path ? ROCArray{Int32}(undef, N, nsamples, B) : nothing
    logprob = want_logprob ? ROCArray{Float32}(undef, nsamples, B) : nothing
    logz = ROCArray{Float32}(undef, B)
    lp = lens === nothing ? Ptr{Int32}(C_NULL) : Ptr{Int32}(pointer(lens))
    check(ccall((:mm_latticesample_f32, LIB), Cint,
        (Ptr{Cvoid}, Ptr{Float32}, Int64, Int64, Ptr{Int32}, Int64, Ptr{Int64}, Ptr{Int32}, Int64, Ptr{Float32}, Int64, Int64, Ptr{Float32},
         Ptr{Int64}, Int64, Int64, Ptr{Int32}, Int64, Int64, Ptr{Float32}, Int64, Ptr{Float32}, Ptr{Cvoid}),
        b.handle, pointer(V), P * N, P, lp, N, pointer(offs), pointer(arcd), n, ex === nothing ? Ptr{Float32}(C_NULL) : pointer(ex),
        nsamples, seed % Int64, pointer(fwd), pointer(rec), N * nsamples, N,
        path === nothing ? Ptr{Int32}(C_NULL) : pointer(path), N * nsamples, N,
        logprob === nothing ? Ptr{Float32}(C_NULL) : pointer(logprob), nsamples, pointer(logz), AMDGPU.stream().stream))
    Array(rec) .+ Int64(1), path === nothing ? nothing : Array(path) .+ Int32(1), logprob === nothing ? nothing : Array(logprob), Array(logz)
end

"""
    totalsum(b::ROCBatch, n) / totalcumsum(b::ROCBatch, n) -> Vector{Float32}

src/algorithms.jl:8-29 for every FSM of the batch (natural-log values of the batch's semiring).
"""
function _totalsum(b::ROCBatch, n::Integer, cumulative::Bool)
    out = ROCArray{Float32}(undef, length(b.fsms))
    check(ccall((:mm_totalsum_f32, LIB), Cint, (Ptr{Cvoid}, Int64, Cint, Ptr{Float32}, Ptr{Cvoid}),
        b.handle, n, cumulative, pointer(out), AMDGPU.stream().stream))
    Array(out)
end
totalsum(b::ROCBatch, n::Integer) = _totalsum(b, n, false)
totalcumsum(b::ROCBatch, n::Integer) = _totalsum(b, n, true)

"""
    last_redo_count(b::ROCBatch) -> Int

How many utterances of the last `pdfposteriors` call the fast kernels handed to the exact ones (computed twice: only
the time differs).  Synchronises the current stream.
"""
function last_redo_count(b::ROCBatch)
    n = Ref{Int64}(0)
    check(ccall((:mm_batch_last_redo_count, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ref{Int64}), b.handle, AMDGPU.stream().stream, n))
    Int(n[])
end

"... and how many of those the float64 exact kernels handed on to the log-domain kernels (normally 0)."
function last_fallback_count(b::ROCBatch)
    n = Ref{Int64}(0)
    check(ccall((:mm_batch_last_fallback_count, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ref{Int64}), b.handle, AMDGPU.stream().stream, n))
    Int(n[])
end
"true if the last `pdfposteriors` call skipped the float32 kernels (the inputs of the call before were hard)."
last_exact_first(b::ROCBatch) = ccall((:mm_batch_last_exact_first, LIB), Cint, (Ptr{Cvoid},), b.handle) != 0
"(workgroups of the team kernels' launches since the last call whose whole team sat on one XCD, all such workgroups): a measurement aid; synchronises the device."
function team_xcd_stats(b::ROCBatch)
    out = zeros(Cint, 2)
    check(ccall((:mm_batch_team_xcd_stats, LIB), Cint, (Ptr{Cvoid}, Ptr{Cint}), b.handle, out))
    Int(out[1]), Int(out[2])
end
"Size the generic entry's workspace (before capturing `pdfposteriors_generic` in a hipGraph)."
reserve_ex!(b::ROCBatch, ::Type{T}, N1::Integer) where T =
    (check(ccall((:mm_batch_reserve_ex, LIB), Cint, (Ptr{Cvoid}, Cint, Int64), b.handle, sizeof(T), N1)); b)

"""
    pdfposteriors_generic(b::ROCBatch{K}, V̂::ROCArray{T,3}, Ĉs = nothing) -> (γ, ttl)

The reference's `pdfposteriors(fsm, V̂s, Ĉs)` (src/inference.jl:145-161) over its whole argument space: any semiring the
FSMs were created with (Log, Tropical, Prob), `T` Float32 or Float64, `V̂` the (P+1) × (N+1) × B stack of matrices as
`expand` or anything else made them (semiring VALUES, `val.(...)`), `Ĉs` `nothing` (every FSM's own one-hot map) or
one sparse matrix per utterance with any number of weighted entries per row.  Returns γ of size B × P × N and ttl.
A plain kernel (alpha and beta materialised like the reference does): correctness first; the fast kernels are behind
`pdfposteriors(b, V, lens)`.
"""
function pdfposteriors_generic(b::ROCBatch{K}, V̂::ROCArray{T,3}, Ĉs = nothing) where {K, T <: Union{Float32, Float64}}
    P1, N1, B = size(V̂)
    B == length(b.fsms) || throw(DimensionMismatch("V̂ holds $B matrices, the batch $(length(b.fsms)) FSMs"))
    # rows of V̂ against the pdfs of the map in force (src/inference.jl:146-150); the C entry checks the same (MM_ERR_DIM)
    for (i, f) in enumerate(b.fsms)
        want = Ĉs === nothing ? f.P1 : size(Ĉs[i], 2)
        P1 == want || throw(DimensionMismatch("V̂ has $P1 rows, the state map of utterance $i has $want pdfs (was expand() applied?)"))
    end
    γ = ROCArray{T}(undef, B, P1 - 1, N1 - 1)
    ttl = ROCArray{T}(undef, B)
    maps = Ptr{Cvoid}[]
    if Ĉs !== nothing
        for Ĉ in Ĉs                                   # CSR of Ĉ = CSC of Ĉ'
            Ct = SparseMatrixCSC(copy(Ĉ'))
            vals = Vector{Float64}(val.(nonzeros(Ct)))
            h = Ref{Ptr{Cvoid}}(C_NULL)
            GC.@preserve Ct vals check(ccall((:mm_statemap_create, LIB), Cint,
                (Cint, Int64, Int32, Int64, Cint, Cint, Cint, Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cvoid}, Ref{Ptr{Cvoid}}),
                semiring_id(K), size(Ĉ, 1), Int32(size(Ĉ, 2)), nnz(Ct), 8, 1, 8,
                pointer(Ct.colptr), pointer(Ct.rowval), pointer(vals), h))
            push!(maps, h[])
        end
    end
    try
        # strides in elements: V̂ (b, n, p) -> p + P1*n + P1*N1*b ; γ (b, n, p) -> b + B*p + B*P*n
        check(ccall((:mm_pdfposteriors_ex, LIB), Cint,
            (Ptr{Cvoid}, Ptr{Ptr{Cvoid}}, Cint, Int32, Ptr{Cvoid}, Int64, Int64, Int64, Ptr{Cvoid}, Int64, Int64, Int64,
             Ptr{Cvoid}, Ptr{Cvoid}),
            b.handle, isempty(maps) ? C_NULL : pointer(maps), sizeof(T), Int32(P1), pointer(V̂), P1 * N1, P1, N1,
            pointer(γ), 1, B * (P1 - 1), B, pointer(ttl), AMDGPU.stream().stream))
        isempty(maps) || AMDGPU.synchronize()           # (the call is asynchronous: the maps must outlive it)
    finally
        foreach(h -> ccall((:mm_statemap_destroy, LIB), Cint, (Ptr{Cvoid},), h), maps)
    end
    γ, ttl
end

"""
    set_exact_policy!(b::ROCBatch, policy::Symbol = :auto)

Which linear-domain kernels a shared-graph batch starts with (mm_batch_set_exact_policy): `:auto` (float32 first; the
wide-exponent kernels first while the last FINISHED call left utterances marked -- read without synchronising, so a pipelined
caller's kernel choice depends on host / device timing), `:f32_first`, `:f64_first` (both: the launches of a call are a
function of the call alone, identical call sequences give identical bits).  Pins the path of `αrecursion` / `βrecursion` too
(`:auto`: the log-domain kernel first while the last export handed it more than half of the utterances; `:f64_first`: that kernel alone).
"""
set_exact_policy!(b::ROCBatch, policy::Symbol = :auto) =
    (check(ccall((:mm_batch_set_exact_policy, LIB), Cint, (Ptr{Cvoid}, Cint), b.handle,
                 policy === :auto ? 0 : policy === :f32_first ? 1 : policy === :f64_first ? 2 : throw(ArgumentError("policy")))); b)

"""
    set_mark_policy!(b::ROCBatch, policy::Symbol = :decide)

What a range mark of the float32 linear-domain kernels means (mm_batch_set_mark_policy): `:decide` -- the finish kernel clears it
when its two criteria say nothing that matters was lost (log γ within 1e-4 relative above ~1e-24, an absolute error below ~1e-27
for smaller posteriors) --, `:keep` -- it always stays and the exact kernels compute the utterance: the relative bar down to 1e-30,
at the price of a second pass on inputs that raise marks.
"""
set_mark_policy!(b::ROCBatch, policy::Symbol = :decide) =
    (check(ccall((:mm_batch_set_mark_policy, LIB), Cint, (Ptr{Cvoid}, Cint), b.handle,
                 policy === :decide ? 0 : policy === :keep ? 1 : throw(ArgumentError("policy")))); b)

"""
    set_gamma_mode!(b::ROCBatch; accumulate = false, scale = 1f0)

What `pdfposteriors(b, V, lens)` does with the posteriors (mm_batch_set_gamma_mode): `γ = scale * γ`, or with `accumulate = true`
`γ_out += scale * γ` into the array passed as `out` -- the numerator call with `scale = -1` on the array the denominator call has just
written leaves the LF-MMI gradient `γ_den - γ_num` (examples/test_cuda.jl:140-152) there without a third pass.  Batches of the wave
kernel only (numerator graphs); others throw `MMError(-4, …)`.
"""
set_gamma_mode!(b::ROCBatch; accumulate::Bool = false, scale::Real = 1f0) =
    (check(ccall((:mm_batch_set_gamma_mode, LIB), Cint, (Ptr{Cvoid}, Cint, Cfloat), b.handle, accumulate ? 1 : 0, Float32(scale))); b)

# ---- the reference's semiring linear algebra on the device (src/linalg.jl): mul! and the sparse-vector broadcast --------------
"""
    ROCSparseCSR{K}(A::SparseMatrixCSC{K})  /  ROCSparseVec{K}(x::SparseVector{K})

What `CuSparseMatrixCSR(adapt(CuArray, A))` / `adapt(CuArray, x)` are on the CUDA path (src/linalg.jl:80-131, test/test_linalg.jl:96):
rowPtr / colVal (`Cint`, 1-based) / nzVal of A on the device.  `LinearAlgebra.mul!(c, A, b)` and `mul!(C, A, B, α, β)` on them are
single calls of the HIP library (mm_spmv / mm_spmm), generic in `K` ∈ {Log, Tropical, Prob}Semiring{Float32 | Float64} like the
reference's methods (src/linalg.jl:163-184, 240-262); dense operands are `ROCArray{K}` (a one-field immutable wrapper around a
float: bit-identical to an array of floats).
"""
struct ROCSparseCSR{K}
    rowPtr::ROCVector{Cint}
    colVal::ROCVector{Cint}
    nzVal::ROCVector{K}
    dims::NTuple{2, Int}
end
function ROCSparseCSR(A::SparseMatrixCSC{K}) where K
    At = SparseMatrixCSC(copy(A'))                     # CSC of A' = CSR of A
    ROCSparseCSR{K}(ROCArray(Cint.(At.colptr)), ROCArray(Cint.(At.rowval)), ROCArray(nonzeros(At)), size(A))
end
Base.size(A::ROCSparseCSR) = A.dims
Base.size(A::ROCSparseCSR, i::Integer) = A.dims[i]
struct ROCSparseVec{K}
    nzInd::ROCVector{Cint}
    nzVal::ROCVector{K}
    n::Int
end
ROCSparseVec(x::SparseVector{K}) where K = ROCSparseVec{K}(ROCArray(Cint.(SparseArrays.nonzeroinds(x))), ROCArray(nonzeros(x)), length(x))
_floatbytes(::Type{K}) where K = sizeof(K)              # K wraps one float

function LinearAlgebra.mul!(c::ROCVector{K}, A::ROCSparseCSR{K}, b::ROCVector{K}) where K
    check(ccall((:mm_spmv, LIB), Cint,
        (Cint, Cint, Int64, Int64, Int64, Ptr{Cint}, Ptr{Cint}, Cint, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Int64, Ptr{Cvoid}),
        semiring_id(K), _floatbytes(K), size(A, 1), size(A, 2), length(A.nzVal), pointer(A.rowPtr), pointer(A.colVal), 1,
        pointer(A.nzVal), pointer(b), length(b), pointer(c), length(c), AMDGPU.stream().stream))
    c
end
function LinearAlgebra.mul!(C::ROCMatrix{K}, A::ROCSparseCSR{K}, B::ROCMatrix{K}, α::Number = true, β::Number = false) where K
    check(ccall((:mm_spmm, LIB), Cint,
        (Cint, Cint, Int64, Int64, Int64, Ptr{Cint}, Ptr{Cint}, Cint, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Int64, Int64, Ptr{Cvoid}, Int64, Int64,
         Int64, Cdouble, Ptr{Cvoid}),
        semiring_id(K), _floatbytes(K), size(A, 1), size(A, 2), length(A.nzVal), pointer(A.rowPtr), pointer(A.colVal), 1,
        pointer(A.nzVal), pointer(B), size(B, 1), size(B, 2), stride(B, 2), pointer(C), size(C, 1), size(C, 2), stride(C, 2),
        Float64(β), AMDGPU.stream().stream))
    C
end
"elmul!(out, y, x::ROCSparseVec) / eldiv!(out, x::ROCSparseVec, y) (src/linalg.jl:287-328): out = zero(K), out[i] = x[i] ⊗ y[i] (⊘) at x's stored entries."
function _svdv!(op::Integer, out::ROCVector{K}, x::ROCSparseVec{K}, y::ROCVector{K}) where K
    check(ccall((:mm_svdv, LIB), Cint,
        (Cint, Cint, Cint, Int64, Int64, Ptr{Cint}, Cint, Ptr{Cvoid}, Ptr{Cvoid}, Int64, Ptr{Cvoid}, Int64, Ptr{Cvoid}),
        semiring_id(K), _floatbytes(K), op, x.n, length(x.nzVal), pointer(x.nzInd), 1, pointer(x.nzVal), pointer(y), length(y),
        pointer(out), length(out), AMDGPU.stream().stream))
    out
end
elmul!(out::ROCVector{K}, y::ROCVector{K}, x::ROCSparseVec{K}) where K = _svdv!(0, out, x, y)
eldiv!(out::ROCVector{K}, x::ROCSparseVec{K}, y::ROCVector{K}) where K = _svdv!(1, out, x, y)

"""
    set_rccl(lib)

Tell the engine which RCCL the communicators passed to `allreduce_logz` / `allgather_ttl` belong to: the handle
`Libdl.dlopen` returned for it (Julia opens libraries with local visibility, so the engine cannot find RCCL among the
process's global symbols; it never opens an RCCL of its own).
"""
set_rccl(lib::Ptr{Cvoid}) = check(ccall((:mm_set_rccl, LIB), Cint, (Ptr{Cvoid},), lib))
set_rccl(path::AbstractString) = set_rccl(Libdl.dlopen(path))

"No float atomics in the item kernel (the wave kernel, the default numerator path, is deterministic anyway): bit-identical γ on every run."
set_deterministic!(b::ROCBatch, on::Bool = true) =
    (check(ccall((:mm_batch_set_deterministic, LIB), Cint, (Ptr{Cvoid}, Cint), b.handle, on ? 1 : 0)); b)

"""
    set_posterior_floor!(b::ROCBatch, floor = 1f-30)

Posteriors below `floor` may come out as 0 from the fast (linear-domain) kernels; the default keeps every posterior
above 1e-30 and sends utterances with sharp emissions to the exact kernels (~1.4x the time since round 5; 3-6x before).
`1f-12` keeps them on the fast path (LF-MMI gradients do not see the difference).
"""
set_posterior_floor!(b::ROCBatch, floor::Real = 1f-30) =
    (check(ccall((:mm_batch_set_posterior_floor, LIB), Cint, (Ptr{Cvoid}, Cfloat), b.handle, Float32(floor))); b)

"""
    allreduce_logz(comm, ttl::ROCVector{Float32}) -> Float64
    allgather_ttl(comm, ttl::ROCVector{Float32}, Bmax, world) -> Matrix{Float32}   (Bmax × world)

The only exchange of a sharded batch (utterances are independent: src/fsmops.jl:28-36): the total log-likelihood
the LF-MMI loss consumes (examples/test_cuda.jl:140-152).  `comm` is an RCCL communicator handle (ncclComm_t) of this
process, one process per GPU; call `set_rccl` once with the library it was made with.  `world` = ranks of `comm`.
"""
function allreduce_logz(comm::Ptr{Cvoid}, ttl::ROCVector{Float32})
    s = ROCArray{Float64}(undef, 1)
    check(ccall((:mm_allreduce_logz, LIB), Cint, (Ptr{Cvoid}, Ptr{Float32}, Int64, Ptr{Float64}, Ptr{Cvoid}),
        comm, pointer(ttl), length(ttl), pointer(s), AMDGPU.stream().stream))
    Array(s)[1]
end
function allgather_ttl(comm::Ptr{Cvoid}, ttl::ROCVector{Float32}, Bmax::Integer, world::Integer)
    pad = ROCArray(fill(-Inf32, Bmax))
    copyto!(pad, 1, ttl, 1, length(ttl))
    out = ROCArray{Float32}(undef, world * Bmax)
    check(ccall((:mm_allgather_ttl, LIB), Cint, (Ptr{Cvoid}, Ptr{Float32}, Int64, Ptr{Float32}, Ptr{Cvoid}),
        comm, pointer(pad), Bmax, pointer(out), AMDGPU.stream().stream))
    reshape(Array(out), Bmax, world)
end

end # module
