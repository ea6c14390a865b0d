# PioranHIP.jl — the Julia side of the drop-in boundary (ccall only; no CUDA.jl / AMDGPU.jl).
#
# This is the binding a Pioran.jl maintainer adds to route the ScalableGP log-likelihood to
# libpioran_hip.so.  It overrides nothing for non-Float64 element types, so ForwardDiff Duals
# (Turing/NUTS, test/test_likelihood.jl:55) keep flowing through the original Julia `logl`.
#
# NOTE: the build image has no `julia`, so this file has never been parsed by a Julia front-end; the identical C ABI is
# exercised from Python (pioran.jl_amd/_lib.py), from plain C (tests/cabi_driver.c) and by the GPU parity tests, and
# tests/test_host.py::test_julia_shim_matches_header checks every ccall here against include/pioran_hip.h (symbol,
# argument count, integer / pointer kinds).  See INTEGRATION.md.
module PioranHIP

using LinearAlgebra
using Statistics
using Pioran
import Pioran: log_likelihood, SumOfCelerite, SemiSeparable, CARMA, celerite_coefs
import ChainRulesCore

const LIB = get(ENV, "PIORAN_HIP_LIB", "libpioran_hip")
const ABI_VERSION = 7

# PIORAN_BACKEND=julia keeps every call on Pioran's own Julia code (the escape hatch a deployment wants when no GPU is
# visible or for A/B comparisons); anything else (default "hip") routes Float64 calls to libpioran_hip.so.
# (USE_HIP, MIN_ROWS, MIN_STEPS: read from ENV in __init__, i.e. when the package is LOADED — module-level initialisers run at precompile time
#  and would bake the build machine's environment into the package cache.  LIB stays a const: ccall wants a constant library name; set
#  PIORAN_HIP_LIB before precompiling, or put the library on the loader's path.)
const USE_HIP = Ref(true)
# A drop-in must not be slower than what it replaces.  One scalar evaluation on the GPU walks a short series as a serial chain at ~0.15 us per
# step whatever the term count, Pioran.logl on one CPU core costs ~0.04 us per step and ROW (N = 8192: j = 2 terms 0.60 ms, j = 4 1.31 ms, j = 8
# 2.6 ms on the bench host; the reference's own figure: 0.85 / 1.6 / 3.7 ms — benchmark/benchmarks.jl:76-91, bench.py
# "reference_benchmark_grid_N8192").  So scalar calls with fewer than PIORAN_HIP_MIN_ROWS rows (R = 2 J; default 9, i.e. up to four terms)
# stay on Pioran's own code — unless the series is long: from PIORAN_HIP_MIN_STEPS steps on (default 3072) the library's time-parallel
# family (celerite_tp.hip: segments of the series on different CUs; round 6: boundary phase as a scan) is ahead of one core at every term count
# (N = 8192: j = 2 0.19 ms, j = 4 0.18 ms; N = 4096: 0.21 / 0.17 ms against 0.29 / 0.60 on one core).  Batched calls (logpdf_batch and friends) always use the GPU.  PIORAN_HIP_MIN_ROWS = 0 sends everything to the GPU.
const MIN_ROWS = Ref(9)
const MIN_STEPS = Ref(3072)
# rows the kernels execute: two per term, one for a term with b = d = 0 (Exp / DRW terms: src/Exp.jl:29-33, the DRW half of DRWCelerite src/psd.jl:270-273)
active_rows(b, d) = 2 * length(b) - count(i -> iszero(b[i]) && iszero(d[i]), eachindex(b))
use_hip_scalar(nrows::Integer, nsteps::Integer) = USE_HIP[] && (nrows >= MIN_ROWS[] || nsteps >= MIN_STEPS[])

function __init__()
    USE_HIP[] = lowercase(get(ENV, "PIORAN_BACKEND", "hip")) != "julia"
    MIN_ROWS[] = parse(Int, get(ENV, "PIORAN_HIP_MIN_ROWS", "9"))
    MIN_STEPS[] = parse(Int, get(ENV, "PIORAN_HIP_MIN_STEPS", "3072"))
    USE_HIP[] || return
    v = ccall((:pioran_abi_version, LIB), Cint, ())
    v == ABI_VERSION || error("libpioran_hip.so has ABI version $v, PioranHIP.jl was written for $ABI_VERSION")
end

struct PioranHIPError <: Exception
    code::Cint
    msg::String
end

function check(rc::Cint)
    rc == 0 && return
    msg = unsafe_string(ccall((:pioran_strerror, LIB), Cstring, (Cint,), rc))
    throw(PioranHIPError(rc, msg))
end

# ---- context: one per Julia process / MPI rank / Distributed worker (device = rank % ngpu) ---------
# Julia does not order finalizers: a Dataset may be finalized after its Context.  pioran_dataset_destroy dereferences the
# context, so the Context keeps the handles of its live data sets and destroys THEM first; a Dataset whose context is
# already gone only forgets its handle.
mutable struct Context
    h::Ptr{Cvoid}
    datasets::Set{Ptr{Cvoid}}
    function Context(device::Integer = 0)
        r = Ref{Ptr{Cvoid}}(C_NULL)
        check(ccall((:pioran_ctx_create, LIB), Cint, (Cint, Ref{Ptr{Cvoid}}), device, r))
        ctx = new(r[], Set{Ptr{Cvoid}}())
        finalizer(close!, ctx)
        return ctx
    end
end

function close!(ctx::Context)
    ctx.h == C_NULL && return
    for d in ctx.datasets
        ccall((:pioran_dataset_destroy, LIB), Cint, (Ptr{Cvoid},), d)
    end
    empty!(ctx.datasets)
    ccall((:pioran_ctx_destroy, LIB), Cint, (Ptr{Cvoid},), ctx.h)
    ctx.h = C_NULL
    return
end

# diagnostic switches of a context (pioran_ctx_set_option: "no_split", "workspace_limit_mb", "dense_old_chain", ...) and the FP64 FMA rate
# the device sustains right now (TFLOP/s; the measured ceiling of any FP64 vector kernel on this box)
set_option!(ctx::Context, key::AbstractString, value::Union{Nothing, AbstractString} = "1") =
    check(ccall((:pioran_ctx_set_option, LIB), Cint, (Ptr{Cvoid}, Cstring, Cstring), ctx.h, key, value === nothing ? C_NULL : value))
function fp64_probe(ctx::Context = default_context(); waves_per_simd::Integer = 2, ms::Real = 10.0)
    out = Ref{Cdouble}(0.0)
    check(ccall((:pioran_ctx_fp64_probe, LIB), Cint, (Ptr{Cvoid}, Cint, Cdouble, Ref{Cdouble}), ctx.h, waves_per_simd, ms, out))
    return out[]
end

const DEFAULT_CTX = Ref{Union{Nothing, Context}}(nothing)
default_context() = (DEFAULT_CTX[] === nothing && (DEFAULT_CTX[] = Context(parse(Int, get(ENV, "PIORAN_HIP_DEVICE", "0")))); DEFAULT_CTX[])

# ---- scalar drop-in: logl(a, b, c, d, τ, y, σ2)  (src/celerite_solver.jl:312-334) -------------------
function logl_hip(a::Vector{Float64}, b::Vector{Float64}, c::Vector{Float64}, d::Vector{Float64},
                  τ::Vector{Float64}, y::Vector{Float64}, σ2::Vector{Float64}; ctx = default_context())
    out = Ref{Cdouble}(NaN)
    status = Ref{Int32}(0)
    GC.@preserve a b c d τ y σ2 begin
        check(ccall((:pioran_celerite_logl, LIB), Cint,
                    (Ptr{Cvoid}, Int64, Int64, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble},
                     Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ref{Cdouble}, Ref{Int32}),
                    ctx.h, length(τ), length(a), a, b, c, d, τ, y, σ2, out, status))
    end
    # status 2: the reference throws DomainError from log(D[1] < 0) (src/celerite_solver.jl:126)
    status[] == 2 && throw(DomainError(out[], "log-likelihood is not finite: covariance not positive definite"))
    return out[]
end

# Float64-only methods: everything else (Duals, BigFloat, views ...) falls through to Pioran's own code.
# The three methods of src/celerite_solver.jl:262-294, same solver switch and error text.
function log_likelihood(cov::SumOfCelerite, τ::Vector{Float64}, y::Vector{Float64}, σ2::Vector{Float64}; solver = :celerite)
    (solver == :celerite || solver == :celerite_matrix) ||
        error("solver $solver not recognised, use either :celerite or :celerite_matrix")
    if use_hip_scalar(active_rows(cov.b, cov.d), length(τ)) && eltype(cov.a) === Float64
        return logl_hip(collect(cov.a), collect(cov.b), collect(cov.c), collect(cov.d), τ, y, σ2)
    end
    return Pioran.logl(cov.a, cov.b, cov.c, cov.d, τ, y, σ2)
end

# CARMA (:272-282) and any other SemiSeparable kernel (:284-294): celerite_coefs, then real(logl(...))
function _log_likelihood_coefs(cov, τ::Vector{Float64}, y::Vector{Float64}, σ2::Vector{Float64}, solver)
    (solver == :celerite || solver == :celerite_matrix) ||
        error("solver $solver not recognised, use either :celerite or :celerite_matrix")
    a, b, c, d = celerite_coefs(cov)
    if use_hip_scalar(active_rows(b, d), length(τ)) && all(v -> eltype(v) <: Union{Float64, ComplexF64}, (a, b, c, d)) && all(v -> all(iszero, imag.(v)), (a, b, c, d))
        return logl_hip(collect(Float64, real.(a)), collect(Float64, real.(b)), collect(Float64, real.(c)), collect(Float64, real.(d)), τ, y, σ2)
    end
    return real(Pioran.logl(a, b, c, d, τ, y, σ2))
end
log_likelihood(cov::CARMA, τ::Vector{Float64}, y::Vector{Float64}, σ2::Vector{Float64}; solver = :celerite) =
    _log_likelihood_coefs(cov, τ, y, σ2, solver)
log_likelihood(cov::SemiSeparable, τ::Vector{Float64}, y::Vector{Float64}, σ2::Vector{Float64}; solver = :celerite) =
    _log_likelihood_coefs(cov, τ, y, σ2, solver)

# Reverse rule for the scalar likelihood: Zygote / ReverseDiff-based samplers (and Turing with an rrule-aware backend) get
# the GPU gradient instead of pushing Duals through Pioran.logl.  Cotangents for (a, b, c, d, y, σ2); τ is data.
function ChainRulesCore.rrule(::typeof(logl_hip), a::Vector{Float64}, b::Vector{Float64}, c::Vector{Float64}, d::Vector{Float64},
                              τ::Vector{Float64}, y::Vector{Float64}, σ2::Vector{Float64}; ctx = default_context())
    ds = Dataset(τ, y, σ2; ctx = ctx)
    g = try
        logpdf_grad_batch(ds, reshape(a, :, 1), reshape(b, :, 1), c, d; series = true)
    finally
        close!(ds)
    end
    g.status[1] == 2 && throw(DomainError(g.logl[1], "log-likelihood is not finite: covariance not positive definite"))
    function logl_pullback(Δ)
        NT = ChainRulesCore.NoTangent()
        return (NT, Δ .* vec(g.grad_a), Δ .* vec(g.grad_b), Δ .* vec(g.grad_c), Δ .* vec(g.grad_d), NT, Δ .* vec(g.grad_y), Δ .* vec(g.grad_σ²))
    end
    return g.logl[1], logl_pullback
end

# ---- data set handle + batched entry (the reference has no batch dimension) ---------------------------
mutable struct Dataset
    h::Ptr{Cvoid}
    N::Int
    ctx::Context
    function Dataset(t::Vector{Float64}, y::Vector{Float64}, σ2::Vector{Float64}; ctx = default_context())
        r = Ref{Ptr{Cvoid}}(C_NULL)
        GC.@preserve t y σ2 check(ccall((:pioran_dataset_create, LIB), Cint,
            (Ptr{Cvoid}, Int64, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ref{Ptr{Cvoid}}), ctx.h, length(t), t, y, σ2, r))
        ds = new(r[], length(t), ctx)
        push!(ctx.datasets, ds.h)
        finalizer(close!, ds)
        return ds
    end
end

function close!(ds::Dataset)
    ds.h == C_NULL && return
    if ds.ctx.h != C_NULL && ds.h in ds.ctx.datasets      # context still alive: it has not destroyed this handle yet
        delete!(ds.ctx.datasets, ds.h)
        ccall((:pioran_dataset_destroy, LIB), Cint, (Ptr{Cvoid},), ds.h)
    end
    ds.h = C_NULL
    return
end

"""
    logpdf_batch(ds, A, B, c, d; μ, ν, Y, S2)

`A`, `B`: `J × nbatch` matrices (one column per draw, Julia column-major = the ABI's `[B][J]`);
`c`, `d`: length-`J` vectors shared by all draws (as produced by `approx`, src/psd.jl:250,266-267) or
`J × nbatch` matrices.  Returns `(logl::Vector{Float64}, status::Vector{Int32})`.
This is what an ultranest `vectorized=true` callback calls once per batch of live points.
"""
function logpdf_batch(ds::Dataset, A::Matrix{Float64}, B::Matrix{Float64}, c::VecOrMat{Float64}, d::VecOrMat{Float64};
                      μ::Union{Nothing, Vector{Float64}} = nothing, ν::Union{Nothing, Vector{Float64}} = nothing,
                      Y::Union{Nothing, Matrix{Float64}} = nothing, S2::Union{Nothing, Matrix{Float64}} = nothing)
    J, nb = size(A)
    out = Vector{Float64}(undef, nb)
    status = zeros(Int32, nb)
    p(x) = x === nothing ? Ptr{Cdouble}(C_NULL) : pointer(x)
    GC.@preserve A B c d μ ν Y S2 out status begin
        check(ccall((:pioran_celerite_logl_batch, LIB), Cint,
                    (Ptr{Cvoid}, Int64, Int64, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cint,
                     Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Int32}),
                    ds.h, nb, J, A, B, c, d, c isa Vector ? 1 : 0, p(μ), p(ν), p(Y), p(S2), out, status))
    end
    return out, status
end

"""
    logpdf_batch_shift(ds, A, B, c, d, shift; μ, ν)

The shifted log-flux models (docs/src/ultranest.md:199-205): `ds` holds the raw flux `y` and `yerr.^2`; draw `b` is
evaluated on `log.(y .- shift[b])` with variances `ν[b] .* yerr.^2 ./ (y .- shift[b]).^2`, transformed on the GPU.
"""
function logpdf_batch_shift(ds::Dataset, A::Matrix{Float64}, B::Matrix{Float64}, c::VecOrMat{Float64}, d::VecOrMat{Float64},
                            shift::Vector{Float64}; μ::Union{Nothing, Vector{Float64}} = nothing,
                            ν::Union{Nothing, Vector{Float64}} = nothing)
    J, nb = size(A)
    out = Vector{Float64}(undef, nb)
    status = zeros(Int32, nb)
    p(x) = x === nothing ? Ptr{Cdouble}(C_NULL) : pointer(x)
    GC.@preserve A B c d μ ν shift out status begin
        check(ccall((:pioran_celerite_logl_batch_shift, LIB), Cint,
                    (Ptr{Cvoid}, Int64, Int64, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cint,
                     Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Int32}),
                    ds.h, nb, J, A, B, c, d, c isa Vector ? 1 : 0, p(μ), p(ν), shift, out, status))
    end
    return out, status
end

"""
    logpdf_batch_theta(ds, model, θ, norm, f_min, f_max, n_components; basis, μ, ν, shift, ...)

θ → log L in one call: `approx` (src/psd.jl:214-289) runs on the GPU in front of the scan, so only the sampled parameters
cross the boundary.  `model`: `:SingleBendingPowerLaw` (`θ` is `3 × nbatch`: α₁, f₁, α₂) or `:DoubleBendingPowerLaw`
(`5 × nbatch`); `norm`: the `norm` argument of `approx` per draw; `basis`: `"SHO"` or `"DRWCelerite"`.
This is the whole body of an ultranest `vectorized=true` likelihood for the models of docs/src/ultranest.md.
"""
function logpdf_batch_theta(ds::Dataset, model::Symbol, θ::Matrix{Float64}, norm::Vector{Float64}, f_min::Real, f_max::Real,
                            n_components::Integer; basis::String = "SHO", is_integrated_power::Bool = true,
                            S_low::Real = 20.0, S_high::Real = 20.0, μ::Union{Nothing, Vector{Float64}} = nothing,
                            ν::Union{Nothing, Vector{Float64}} = nothing, shift::Union{Nothing, Vector{Float64}} = nothing,
                            qpo::Union{Nothing, Array{Float64, 3}} = nothing)   # 3 × n_qpo × nbatch: (S₀, f₀, Q) of the QPO features
    m = model === :SingleBendingPowerLaw ? 0 : model === :DoubleBendingPowerLaw ? 1 : error("model $model not supported on the device")
    bs = basis == "SHO" ? 0 : basis == "DRWCelerite" ? 1 : error("basis $basis not supported on the device")
    size(θ, 1) == (m == 0 ? 3 : 5) || error("θ must be $(m == 0 ? 3 : 5) × nbatch")
    nb = size(θ, 2)
    nq = qpo === nothing ? 0 : size(qpo, 2)
    out = Vector{Float64}(undef, nb)
    status = zeros(Int32, nb)
    p(x) = x === nothing ? Ptr{Cdouble}(C_NULL) : pointer(x)
    GC.@preserve θ norm μ ν shift qpo out status begin
        check(ccall((:pioran_logpdf_batch_theta, LIB), Cint,
                    (Ptr{Cvoid}, Int64, Cint, Int64, Cint, Cint, Cdouble, Cdouble, Cdouble, Cdouble, Ptr{Cdouble}, Ptr{Cdouble},
                     Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Int64, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Int32}, Ptr{Cdouble}, Ptr{Cdouble}),
                    ds.h, nb, m, n_components, bs, is_integrated_power ? 1 : 0, f_min, f_max, S_low, S_high, θ, norm,
                    p(μ), p(ν), p(shift), nq, p(qpo), out, status, C_NULL, C_NULL))
    end
    return out, status
end

"""
    logpdf_theta_grad_batch(ds, model, θ, norm, f_min, f_max, n_components; basis, μ, ν, shift, coef_grads, ...)

Value and gradient with respect to the sampled parameters in one device call: `approx`, the reverse mode of the likelihood and the
reverse mode of `approx` all run on the GPU; `θ` (`P × nbatch`), `norm`, `μ`, `ν`, `shift` go in and `grad_θ` (`P × nbatch`),
`grad_norm`, `grad_ν`, `grad_μ`, `grad_shift` (each `nothing` when its input is) come out.  Continuum models; with QPO features: `logpdf_theta_qpo_grad_batch`.
`coef_grads = true` also returns the intermediate `grad_a`, `grad_b` (`J × nbatch`).
"""
function logpdf_theta_grad_batch(ds::Dataset, model::Symbol, θ::Matrix{Float64}, norm::Vector{Float64}, f_min::Real, f_max::Real,
                                 n_components::Integer; basis::String = "SHO", is_integrated_power::Bool = true,
                                 S_low::Real = 20.0, S_high::Real = 20.0, μ::Union{Nothing, Vector{Float64}} = nothing,
                                 ν::Union{Nothing, Vector{Float64}} = nothing, shift::Union{Nothing, Vector{Float64}} = nothing,
                                 coef_grads::Bool = false)
    m = model === :SingleBendingPowerLaw ? 0 : model === :DoubleBendingPowerLaw ? 1 : error("model $model not supported on the device")
    bs = basis == "SHO" ? 0 : basis == "DRWCelerite" ? 1 : error("basis $basis not supported on the device")
    size(θ, 1) == (m == 0 ? 3 : 5) || error("θ must be $(m == 0 ? 3 : 5) × nbatch")
    nb = size(θ, 2)
    J = bs == 0 ? n_components : 2 * n_components
    out = Vector{Float64}(undef, nb); status = zeros(Int32, nb)
    gθ = Matrix{Float64}(undef, size(θ, 1), nb); gn = Vector{Float64}(undef, nb)
    like(x) = x === nothing ? nothing : Vector{Float64}(undef, nb)
    gν = like(ν); gμ = like(μ); gs = like(shift)
    ga = coef_grads ? Matrix{Float64}(undef, J, nb) : nothing; gb = coef_grads ? Matrix{Float64}(undef, J, nb) : nothing
    p(x) = x === nothing ? Ptr{Cdouble}(C_NULL) : pointer(x)
    GC.@preserve θ norm μ ν shift out status gθ gn gν gμ gs ga gb begin
        check(ccall((:pioran_logpdf_batch_theta_grad, LIB), Cint,
                    (Ptr{Cvoid}, Int64, Cint, Int64, Cint, Cint, Cdouble, Cdouble, Cdouble, Cdouble, Ptr{Cdouble}, Ptr{Cdouble},
                     Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Int32}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble},
                     Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
                    ds.h, nb, m, n_components, bs, is_integrated_power ? 1 : 0, f_min, f_max, S_low, S_high, θ, norm,
                    p(μ), p(ν), p(shift), out, status, gθ, gn, p(gν), p(gμ), p(gs), p(ga), p(gb)))
    end
    return (logl = out, status = status, grad_θ = gθ, grad_norm = gn, grad_ν = gν, grad_μ = gμ, grad_shift = gs, grad_a = ga, grad_b = gb)
end

"""
    approx_vjp_batch(model, θ, norm, grad_a, grad_b, f_min, f_max, n_components; basis, ctx, ...)

The reverse mode of `approx` alone, on the GPU — what an `rrule` for `approx` returns for the cotangents `grad_a`, `grad_b`
(`J × nbatch`) of the celerite coefficients: `(grad_θ, grad_norm)`.
"""
function approx_vjp_batch(model::Symbol, θ::Matrix{Float64}, norm::Vector{Float64}, grad_a::Matrix{Float64}, grad_b::Matrix{Float64},
                          f_min::Real, f_max::Real, n_components::Integer; basis::String = "SHO", is_integrated_power::Bool = true,
                          S_low::Real = 20.0, S_high::Real = 20.0, ctx = default_context())
    m = model === :SingleBendingPowerLaw ? 0 : model === :DoubleBendingPowerLaw ? 1 : error("model $model not supported on the device")
    bs = basis == "SHO" ? 0 : basis == "DRWCelerite" ? 1 : error("basis $basis not supported on the device")
    size(θ, 1) == (m == 0 ? 3 : 5) || error("θ must be $(m == 0 ? 3 : 5) × nbatch")
    nb = size(θ, 2)
    size(grad_a) == size(grad_b) == ((bs == 0 ? 1 : 2) * n_components, nb) || error("grad_a, grad_b must be J × nbatch")
    gθ = Matrix{Float64}(undef, size(θ, 1), nb); gn = Vector{Float64}(undef, nb)
    GC.@preserve θ norm grad_a grad_b gθ gn begin
        check(ccall((:pioran_approx_vjp_batch, LIB), Cint,
                    (Ptr{Cvoid}, Int64, Cint, Int64, Cint, Cint, Cdouble, Cdouble, Cdouble, Cdouble, Ptr{Cdouble}, Ptr{Cdouble},
                     Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
                    ctx.h, nb, m, n_components, bs, is_integrated_power ? 1 : 0, f_min, f_max, S_low, S_high, θ, norm,
                    grad_a, grad_b, gθ, gn))
    end
    return gθ, gn
end

"""
    logpdf_theta_qpo_grad_batch(ds, model, θ, norm, qpo, f_min, f_max, n_components; basis, μ, ν, shift, coef_grads, ...)

Value and gradient with respect to the sampled parameters of a continuum + QPO model in one call: `qpo` is `3 × n_qpo × nbatch`
(S₀, f₀, Q), `1 ≤ n_qpo ≤ 8`; besides `logpdf_theta_grad_batch`'s results `grad_qpo` (`3 × n_qpo × nbatch`) comes out.  Every draw
has its own (c, d): the reverse mode is `logl_grad`'s for per-draw tables.  A draw the reference could not evaluate (non-finite
parameters, f₀ ≤ 0, Q ≤ 1/2) has status 3, `logl = -Inf` and zero gradients.  `coef_grads = true` also returns the coefficients
`coef_a … coef_d` and their gradients `grad_a … grad_d` (`Jt × nbatch`, `Jt = J + n_qpo`).
"""
function logpdf_theta_qpo_grad_batch(ds::Dataset, model::Symbol, θ::Matrix{Float64}, norm::Vector{Float64}, qpo::Array{Float64, 3},
                                     f_min::Real, f_max::Real, n_components::Integer; basis::String = "SHO",
                                     is_integrated_power::Bool = true, S_low::Real = 20.0, S_high::Real = 20.0,
                                     μ::Union{Nothing, Vector{Float64}} = nothing, ν::Union{Nothing, Vector{Float64}} = nothing,
                                     shift::Union{Nothing, Vector{Float64}} = nothing, coef_grads::Bool = false)
    m = model === :SingleBendingPowerLaw ? 0 : model === :DoubleBendingPowerLaw ? 1 : error("model $model not supported on the device")
    bs = basis == "SHO" ? 0 : basis == "DRWCelerite" ? 1 : error("basis $basis not supported on the device")
    size(θ, 1) == (m == 0 ? 3 : 5) || error("θ must be $(m == 0 ? 3 : 5) × nbatch")
    nb = size(θ, 2)
    size(qpo, 1) == 3 && size(qpo, 3) == nb || error("qpo must be 3 × n_qpo × nbatch")
    nq = size(qpo, 2)
    Jt = (bs == 0 ? 1 : 2) * n_components + nq
    out = Vector{Float64}(undef, nb); status = zeros(Int32, nb)
    gθ = Matrix{Float64}(undef, size(θ, 1), nb); gn = Vector{Float64}(undef, nb); gq = Array{Float64, 3}(undef, 3, nq, nb)
    like(x) = x === nothing ? nothing : Vector{Float64}(undef, nb)
    gν = like(ν); gμ = like(μ); gs = like(shift)
    co = [coef_grads ? Matrix{Float64}(undef, Jt, nb) : nothing for _ in 1:8]
    p(x) = x === nothing ? Ptr{Cdouble}(C_NULL) : pointer(x)
    GC.@preserve θ norm qpo μ ν shift out status gθ gn gq gν gμ gs co begin
        check(ccall((:pioran_logpdf_batch_theta_qpo_grad, LIB), Cint,
                    (Ptr{Cvoid}, Int64, Cint, Int64, Cint, Cint, Cdouble, Cdouble, Cdouble, Cdouble, Ptr{Cdouble}, Ptr{Cdouble},
                     Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Int64, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Int32}, Ptr{Cdouble}, Ptr{Cdouble},
                     Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble},
                     Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
                    ds.h, nb, m, n_components, bs, is_integrated_power ? 1 : 0, f_min, f_max, S_low, S_high, θ, norm,
                    p(μ), p(ν), p(shift), nq, qpo, out, status, gθ, gn, gq, p(gν), p(gμ), p(gs),
                    p(co[1]), p(co[2]), p(co[3]), p(co[4]), p(co[5]), p(co[6]), p(co[7]), p(co[8])))
    end
    return (logl = out, status = status, grad_θ = gθ, grad_norm = gn, grad_qpo = gq, grad_ν = gν, grad_μ = gμ, grad_shift = gs,
            coef_a = co[1], coef_b = co[2], coef_c = co[3], coef_d = co[4], grad_a = co[5], grad_b = co[6], grad_c = co[7], grad_d = co[8])
end

"""
    approx_qpo_vjp_batch(model, θ, norm, qpo, grad_a, grad_b, grad_c, grad_d, f_min, f_max, n_components; basis, ctx, ...)

The reverse mode of `approx` with QPO features alone, on the GPU: cotangents `grad_a … grad_d` (`Jt × nbatch`; of `grad_c`, `grad_d`
only the feature rows are read) of the celerite coefficients → `(grad_θ, grad_norm, grad_qpo)`.
"""
function approx_qpo_vjp_batch(model::Symbol, θ::Matrix{Float64}, norm::Vector{Float64}, qpo::Array{Float64, 3}, grad_a::Matrix{Float64},
                              grad_b::Matrix{Float64}, grad_c::Matrix{Float64}, grad_d::Matrix{Float64}, f_min::Real, f_max::Real,
                              n_components::Integer; basis::String = "SHO", is_integrated_power::Bool = true, S_low::Real = 20.0,
                              S_high::Real = 20.0, ctx = default_context())
    m = model === :SingleBendingPowerLaw ? 0 : model === :DoubleBendingPowerLaw ? 1 : error("model $model not supported on the device")
    bs = basis == "SHO" ? 0 : basis == "DRWCelerite" ? 1 : error("basis $basis not supported on the device")
    size(θ, 1) == (m == 0 ? 3 : 5) || error("θ must be $(m == 0 ? 3 : 5) × nbatch")
    nb = size(θ, 2)
    size(qpo, 1) == 3 && size(qpo, 3) == nb || error("qpo must be 3 × n_qpo × nbatch")
    nq = size(qpo, 2)
    size(grad_a) == size(grad_b) == size(grad_c) == size(grad_d) == ((bs == 0 ? 1 : 2) * n_components + nq, nb) ||
        error("grad_a … grad_d must be (J + n_qpo) × nbatch")
    gθ = Matrix{Float64}(undef, size(θ, 1), nb); gn = Vector{Float64}(undef, nb); gq = Array{Float64, 3}(undef, 3, nq, nb)
    GC.@preserve θ norm qpo grad_a grad_b grad_c grad_d gθ gn gq begin
        check(ccall((:pioran_approx_qpo_vjp_batch, LIB), Cint,
                    (Ptr{Cvoid}, Int64, Cint, Int64, Cint, Cint, Cdouble, Cdouble, Cdouble, Cdouble, Ptr{Cdouble}, Ptr{Cdouble}, Int64,
                     Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
                    ctx.h, nb, m, n_components, bs, is_integrated_power ? 1 : 0, f_min, f_max, S_low, S_high, θ, norm, nq, qpo,
                    grad_a, grad_b, grad_c, grad_d, gθ, gn, gq))
    end
    return gθ, gn, gq
end

# ---- CARMA(p, q) models from their sampled parameters (src/CARMA.jl, docs/src/carma.md) ---------------------------------------------------
# Quad form: qa `p × nbatch`, qb `q × nbatch`, the quadratic factors the models sample (rα = quad2roots(qa), β = roots2coeffs(quad2roots(qb)));
# roots form: rα `p × nbatch` ComplexF64, β `(q + 1) × nbatch`.  bounds = (f_lo, f_hi) of check_roots_bounds, or nothing.
_carma_bounds(bounds) = bounds === nothing ? (0.0, 0.0) : (Float64(bounds[1]), Float64(bounds[2]))
_carma_form(in1::Matrix{Float64}) = Cint(0)
_carma_form(in1::Matrix{ComplexF64}) = Cint(1)
function _carma_sizes(p::Integer, q::Integer, in1::Matrix, in2::Matrix{Float64}, norm::Vector{Float64})
    form = _carma_form(in1)
    size(in1, 1) == p || error("the first array must have p = $p rows")
    size(in2, 1) == (form == 0 ? q : q + 1) || error("the second array must have $(form == 0 ? q : q + 1) rows")
    nb = size(in1, 2)
    (size(in2, 2) == nb && length(norm) == nb) || error("one column and one norm per draw")
    return form, nb
end

"""
    carma_coefs_batch(p, q, qa, qb, norm; is_integrated_power, bounds, ctx)          (quad form)
    carma_coefs_batch(p, q, rα, β, norm; ...)                                        (roots form)

`CARMA_celerite_coefs` for a batch on the GPU: `(a, b, c, d)` `J × nbatch`, `J = (p + 1) ÷ 2`, and `flags` (0, or why a draw is rejected: 1 non-finite,
2 not a conjugate pair, 3 a root with real part ≥ 0, 4 outside the bounds; such a draw has (1, 0, 1, 0) in every term).
"""
function carma_coefs_batch(p::Integer, q::Integer, in1::Matrix, in2::Matrix{Float64}, norm::Vector{Float64}; is_integrated_power::Bool = true,
                           bounds = nothing, ctx = default_context())
    form, nb = _carma_sizes(p, q, in1, in2, norm)
    J = (p + 1) ÷ 2
    f_lo, f_hi = _carma_bounds(bounds)
    a, b, c, d = (Matrix{Float64}(undef, J, nb) for _ in 1:4)
    flags = Vector{Int32}(undef, nb)
    GC.@preserve in1 in2 norm a b c d flags begin
        check(ccall((:pioran_carma_coefs_batch, LIB), Cint,
                    (Ptr{Cvoid}, Int64, Cint, Cint, Cint, Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Cdouble, Cdouble, Ptr{Cdouble}, Ptr{Cdouble},
                     Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Int32}),
                    ctx.h, nb, p, q, form, pointer(in1), q == 0 && form == 0 ? C_NULL : pointer(in2), norm, is_integrated_power ? 1 : 0, f_lo, f_hi,
                    a, b, c, d, flags))
    end
    return a, b, c, d, flags
end

"""
    carma_vjp_batch(p, q, qa, qb, norm, grad_a, grad_b, grad_c, grad_d; is_integrated_power, ctx)

The reverse mode of quad2roots and `CARMA_celerite_coefs` on the GPU — what an `rrule` returns for the cotangents of the coefficients
(`J × nbatch` each): `(grad_qa, grad_qb, grad_norm)`.  Rejected draws get exact zeros.
"""
function carma_vjp_batch(p::Integer, q::Integer, qa::Matrix{Float64}, qb::Matrix{Float64}, norm::Vector{Float64}, grad_a::Matrix{Float64},
                         grad_b::Matrix{Float64}, grad_c::Matrix{Float64}, grad_d::Matrix{Float64}; is_integrated_power::Bool = true,
                         ctx = default_context())
    _, nb = _carma_sizes(p, q, qa, qb, norm)
    all(size(g) == ((p + 1) ÷ 2, nb) for g in (grad_a, grad_b, grad_c, grad_d)) || error("the cotangents must be J × nbatch")
    gqa = Matrix{Float64}(undef, p, nb); gqb = Matrix{Float64}(undef, q, nb); gn = Vector{Float64}(undef, nb)
    GC.@preserve qa qb norm grad_a grad_b grad_c grad_d gqa gqb gn begin
        check(ccall((:pioran_carma_vjp_batch, LIB), Cint,
                    (Ptr{Cvoid}, Int64, Cint, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble},
                     Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
                    ctx.h, nb, p, q, qa, q == 0 ? C_NULL : pointer(qb), norm, is_integrated_power ? 1 : 0, grad_a, grad_b, grad_c, grad_d, gqa,
                    q == 0 ? C_NULL : pointer(gqb), gn))
    end
    return gqa, gqb, gn
end

"""
    carma_psd_batch(p, q, in1, in2, norm, f; is_integrated_power, bounds, times_f, ctx)

`evaluate(::CARMA, f)` for a batch on the GPU: `(psd, status)` with `psd` `length(f) × nbatch`; status 3, and NaN in the column, for a rejected draw.
"""
function carma_psd_batch(p::Integer, q::Integer, in1::Matrix, in2::Matrix{Float64}, norm::Vector{Float64}, f::Vector{Float64};
                         is_integrated_power::Bool = true, bounds = nothing, times_f::Bool = false, ctx = default_context())
    form, nb = _carma_sizes(p, q, in1, in2, norm)
    f_lo, f_hi = _carma_bounds(bounds)
    psd = Matrix{Float64}(undef, length(f), nb); status = Vector{Int32}(undef, nb)
    GC.@preserve in1 in2 norm f psd status begin
        check(ccall((:pioran_carma_psd_batch, LIB), Cint,
                    (Ptr{Cvoid}, Int64, Cint, Cint, Cint, Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Cdouble, Cdouble, Int64, Ptr{Cdouble}, Cint,
                     Ptr{Cdouble}, Ptr{Int32}),
                    ctx.h, nb, p, q, form, pointer(in1), q == 0 && form == 0 ? C_NULL : pointer(in2), norm, is_integrated_power ? 1 : 0, f_lo, f_hi,
                    length(f), f, times_f ? 1 : 0, psd, status))
    end
    return psd, status
end

"""
    carma_psd_summary(p, q, in1, in2, norm, f, probs = PPC_QUANTILES; ...)

`carma_psd_batch` with the array left on the device and reduced there: `(quant, status, kept)`, `quant` `length(f) × length(probs)` over the draws with
status 0 — the quantiles `plot_psd_ppc_CARMA` draws (src/plots_diagnostics.jl:832-936).  At most 4096 draws.
"""
function carma_psd_summary(p::Integer, q::Integer, in1::Matrix, in2::Matrix{Float64}, norm::Vector{Float64}, f::Vector{Float64},
                           probs::Vector{Float64} = PPC_QUANTILES; is_integrated_power::Bool = true, bounds = nothing, times_f::Bool = false,
                           ctx = default_context())
    form, nb = _carma_sizes(p, q, in1, in2, norm)
    f_lo, f_hi = _carma_bounds(bounds)
    quant = Matrix{Float64}(undef, length(f), length(probs)); status = Vector{Int32}(undef, nb); kept = Ref{Int32}(-1)
    GC.@preserve in1 in2 norm f probs quant status begin
        check(ccall((:pioran_carma_psd_summary, LIB), Cint,
                    (Ptr{Cvoid}, Int64, Cint, Cint, Cint, Ptr{Cvoid}, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Cdouble, Cdouble, Int64, Ptr{Cdouble}, Cint, Int64,
                     Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Int32}, Ref{Int32}),
                    ctx.h, nb, p, q, form, pointer(in1), q == 0 && form == 0 ? C_NULL : pointer(in2), norm, is_integrated_power ? 1 : 0, f_lo, f_hi,
                    length(f), f, times_f ? 1 : 0, length(probs), probs, quant, status, kept))
    end
    return quant, status, Int(kept[])
end

"""
    psd_ppc_carma(samples_rα, samples_β, samples_norm, samples_ν, t, y, yerr, p, q; plot_f_P, n_frequencies, with_log_transform)

`plot_psd_ppc_CARMA` (src/plots_diagnostics.jl:832-936) as numbers, the samples one per ROW as the reference takes them: the grid, the five quantiles of
the PSD per frequency and the two noise levels.
"""
function psd_ppc_carma(samples_rα::Matrix, samples_β::Matrix{Float64}, samples_norm::Vector{Float64}, samples_ν::Vector{Float64}, t::Vector{Float64},
                       y::Vector{Float64}, yerr::Vector{Float64}, p::Integer, q::Integer; plot_f_P::Bool = false, n_frequencies::Integer = 1000,
                       with_log_transform::Bool = false, ctx = default_context())
    p == size(samples_rα, 2) || error("p=$(p) is not equal to the number of columns in samples_rα=$(size(samples_rα, 2))")
    q + 1 == size(samples_β, 2) || error("q+1=$(q + 1) is not equal to the number of columns in samples_β=$(size(samples_β, 2))")
    dt = diff(t)
    f_min = 1 / (t[end] - t[1]) / 10
    f_max = 1 / minimum(dt) / 2.0 * 10
    f = collect(exp.(range(log(f_min), log(f_max), length = n_frequencies)))
    sq_err = with_log_transform ? (yerr ./ y) .^ 2 : yerr .^ 2
    mean_noise_level = 2 * mean(samples_ν) * mean(sq_err) * mean(dt)
    median_noise_level = 2 * median(samples_ν) * median(sq_err) * median(dt)
    rα = Matrix{ComplexF64}(permutedims(samples_rα)); β = Matrix{Float64}(permutedims(samples_β))
    quant, status, kept = carma_psd_summary(p, q, rα, β, samples_norm, f; times_f = plot_f_P, ctx = ctx)
    return (f = f, psd_quantiles = quant, mean_noise_level = mean_noise_level, median_noise_level = median_noise_level, f_min = f_min, f_max = f_max,
            kept = kept)
end

"""
    logpdf_batch_carma(ds, p, q, qa, qb, norm; is_integrated_power, bounds, μ, ν, shift)

(qa, qb, norm) -> log L in one call for the CARMA models of docs/src/carma.md: the whole body of a vectorised likelihood.  `(out, status)`; a draw the
root checks reject has `out = -Inf` and status 3 (the models' `@addlogprob! -Inf`).
"""
function logpdf_batch_carma(ds::Dataset, p::Integer, q::Integer, qa::Matrix{Float64}, qb::Matrix{Float64}, norm::Vector{Float64};
                            is_integrated_power::Bool = true, bounds = nothing, μ::Union{Nothing, Vector{Float64}} = nothing,
                            ν::Union{Nothing, Vector{Float64}} = nothing, shift::Union{Nothing, Vector{Float64}} = nothing)
    _, nb = _carma_sizes(p, q, qa, qb, norm)
    f_lo, f_hi = _carma_bounds(bounds)
    out = Vector{Float64}(undef, nb); status = zeros(Int32, nb)
    pt(x) = x === nothing ? Ptr{Cdouble}(C_NULL) : pointer(x)
    GC.@preserve qa qb norm μ ν shift out status begin
        check(ccall((:pioran_logpdf_batch_carma, LIB), Cint,
                    (Ptr{Cvoid}, Int64, Cint, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Cdouble, Cdouble, Ptr{Cdouble}, Ptr{Cdouble},
                     Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Int32}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
                    ds.h, nb, p, q, qa, q == 0 ? C_NULL : pointer(qb), norm, is_integrated_power ? 1 : 0, f_lo, f_hi, pt(μ), pt(ν), pt(shift), out,
                    status, C_NULL, C_NULL, C_NULL, C_NULL))
    end
    return out, status
end

"""
    logpdf_carma_grad_batch(ds, p, q, qa, qb, norm; is_integrated_power, bounds, μ, ν, shift, coef_grads)

Value and gradient with respect to the sampled parameters of the CARMA models — what NUTS needs: `grad_qa` (`p × nbatch`), `grad_qb` (`q × nbatch`),
`grad_norm`, `grad_ν`, `grad_μ`, `grad_shift` (each `nothing` when its input is); `coef_grads = true` also returns `grad_a .. grad_d` (`J × nbatch`).
A rejected draw has status 3, `logl = -Inf` and zeros in every gradient column.
"""
function logpdf_carma_grad_batch(ds::Dataset, p::Integer, q::Integer, qa::Matrix{Float64}, qb::Matrix{Float64}, norm::Vector{Float64};
                                 is_integrated_power::Bool = true, bounds = nothing, μ::Union{Nothing, Vector{Float64}} = nothing,
                                 ν::Union{Nothing, Vector{Float64}} = nothing, shift::Union{Nothing, Vector{Float64}} = nothing,
                                 coef_grads::Bool = false)
    _, nb = _carma_sizes(p, q, qa, qb, norm)
    J = (p + 1) ÷ 2
    f_lo, f_hi = _carma_bounds(bounds)
    out = Vector{Float64}(undef, nb); status = zeros(Int32, nb)
    gqa = Matrix{Float64}(undef, p, nb); gqb = Matrix{Float64}(undef, q, nb); gn = Vector{Float64}(undef, nb)
    like(x) = x === nothing ? nothing : Vector{Float64}(undef, nb)
    gν = like(ν); gμ = like(μ); gs = like(shift)
    ga, gb, gc, gd = (coef_grads ? Matrix{Float64}(undef, J, nb) : nothing for _ in 1:4)
    pt(x) = x === nothing ? Ptr{Cdouble}(C_NULL) : pointer(x)
    GC.@preserve qa qb norm μ ν shift out status gqa gqb gn gν gμ gs ga gb gc gd begin
        check(ccall((:pioran_logpdf_batch_carma_grad, LIB), Cint,
                    (Ptr{Cvoid}, Int64, Cint, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Cdouble, Cdouble, Ptr{Cdouble}, Ptr{Cdouble},
                     Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Int32}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble},
                     Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
                    ds.h, nb, p, q, qa, q == 0 ? C_NULL : pointer(qb), norm, is_integrated_power ? 1 : 0, f_lo, f_hi, pt(μ), pt(ν), pt(shift), out,
                    status, gqa, q == 0 ? C_NULL : pointer(gqb), gn, pt(gν), pt(gμ), pt(gs), pt(ga), pt(gb), pt(gc), pt(gd)))
    end
    return (logl = out, status = status, grad_qa = gqa, grad_qb = gqb, grad_norm = gn, grad_ν = gν, grad_μ = gμ, grad_shift = gs, grad_a = ga,
            grad_b = gb, grad_c = gc, grad_d = gd)
end

# ---- in-process farm: ONE Julia process driving several GPUs (no Distributed/MPI launcher needed) ----------------------
mutable struct Farm
    h::Ptr{Cvoid}
    function Farm(devices::Vector{<:Integer}, t::Vector{Float64}, y::Vector{Float64}, σ2::Vector{Float64})
        r = Ref{Ptr{Cvoid}}(C_NULL)
        dev = Vector{Cint}(devices)
        GC.@preserve dev t y σ2 check(ccall((:pioran_farm_create, LIB), Cint,
            (Cint, Ptr{Cint}, Int64, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ref{Ptr{Cvoid}}), length(dev), dev, length(t), t, y, σ2, r))
        f = new(r[])
        finalizer(x -> ccall((:pioran_farm_destroy, LIB), Cint, (Ptr{Cvoid},), x.h), f)
        return f
    end
end

"""
    logpdf_batch(farm, A, B, c, d; μ, ν, shift)

Same arguments as the single-GPU `logpdf_batch`; the draws are cut into contiguous shards, one per listed device, every
device writes its slice of the result directly (draws are independent: no collective).
"""
function logpdf_batch(farm::Farm, A::Matrix{Float64}, B::Matrix{Float64}, c::VecOrMat{Float64}, d::VecOrMat{Float64};
                      μ::Union{Nothing, Vector{Float64}} = nothing, ν::Union{Nothing, Vector{Float64}} = nothing,
                      shift::Union{Nothing, Vector{Float64}} = nothing,
                      Y::Union{Nothing, Matrix{Float64}} = nothing, S2::Union{Nothing, Matrix{Float64}} = nothing)
    J, nb = size(A)
    out = Vector{Float64}(undef, nb)
    status = zeros(Int32, nb)
    p(x) = x === nothing ? Ptr{Cdouble}(C_NULL) : pointer(x)
    if Y !== nothing   # per-draw series, N x nb (a column per draw): CustomMean models, y .- mean_b.(t)
        (S2 !== nothing && shift === nothing) || error("Y and S2 come together, and not with shift")
        GC.@preserve A B c d μ ν Y S2 out status begin
            check(ccall((:pioran_farm_logl_batch_series, LIB), Cint,
                        (Ptr{Cvoid}, Int64, Int64, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cint,
                         Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Int32}),
                        farm.h, nb, J, A, B, c, d, c isa Vector ? 1 : 0, p(μ), p(ν), Y, S2, out, status))
        end
        return out, status
    end
    GC.@preserve A B c d μ ν shift out status begin
        check(ccall((:pioran_farm_logl_batch, LIB), Cint,
                    (Ptr{Cvoid}, Int64, Int64, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cint,
                     Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Int32}),
                    farm.h, nb, J, A, B, c, d, c isa Vector ? 1 : 0, p(μ), p(ν), p(shift), out, status))
    end
    return out, status
end

# ---- posterior mean and simulation: pred / sim of src/celerite_solver.jl:363-483, 515-549 ------------------------------------
"""
    predict_batch(ds, A, B, c, d, τ; μ, ν)

Posterior mean at the times `τ` for every draw (column) of `A`, `B`: what `mean(posterior(f(t, σ²), y), τ)`
(src/scalable_GP.jl:64-72) computes one draw at a time.  `c`, `d`: length-`J` vectors shared by the draws, or `J × nbatch` matrices
(posterior draws of QPO / CARMA / free Celerite models: all draws still go through every kernel in one launch, each with its own
tables).  Ascending `τ` takes the fused evaluation.  Returns an `length(τ) × nbatch` matrix and the status vector.
"""
function predict_batch(ds::Dataset, A::Matrix{Float64}, B::Matrix{Float64}, c::VecOrMat{Float64}, d::VecOrMat{Float64},
                       τ::Vector{Float64}; μ::Union{Nothing, Vector{Float64}} = nothing, ν::Union{Nothing, Vector{Float64}} = nothing)
    J, nb = size(A)
    out = Matrix{Float64}(undef, length(τ), nb)      # column-major = the ABI's [B][M]
    status = zeros(Int32, nb)
    p(x) = x === nothing ? Ptr{Cdouble}(C_NULL) : pointer(x)
    GC.@preserve A B c d μ ν τ out status begin
        check(ccall((:pioran_celerite_predict, LIB), Cint,
                    (Ptr{Cvoid}, Int64, Int64, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Ptr{Cdouble}, Ptr{Cdouble},
                     Int64, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Int32}),
                    ds.h, nb, J, A, B, c, d, c isa Vector ? 1 : 0, p(μ), p(ν), length(τ), τ, out, status))
    end
    return out, status
end

"""
    predict_var(ds, A, B, c, d, τ; ν)

Posterior variance of the latent process at the times `τ` (any order) for every draw (column) of `A`, `B`, through the celerite
factorisation in O((N + M) R²): the diagonal that `std(posterior(f(t, σ²), y), τ)` (src/scalable_GP.jl:103-104) takes from a dense
`predict_cov`.  At most 64 active rows.  The error is below 5e-15 `k(0)`, `k(0) = sum(a)`, on well-conditioned draws and reaches 8e-12 `k(0)` at `N = 1000` on draws with `ν min σ² / k(0)` near 1e-10.  Returns an `length(τ) × nbatch`
matrix and the status vector (2 and NaN where a draw's factorisation is not positive definite).
"""
function predict_var(ds::Dataset, A::Matrix{Float64}, B::Matrix{Float64}, c::VecOrMat{Float64}, d::VecOrMat{Float64},
                     τ::Vector{Float64}; ν::Union{Nothing, Vector{Float64}} = nothing)
    J, nb = size(A)
    out = Matrix{Float64}(undef, length(τ), nb)      # column-major = the ABI's [B][M]
    status = zeros(Int32, nb)
    p(x) = x === nothing ? Ptr{Cdouble}(C_NULL) : pointer(x)
    GC.@preserve A B c d ν τ out status begin
        check(ccall((:pioran_celerite_predict_var, LIB), Cint,
                    (Ptr{Cvoid}, Int64, Int64, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Ptr{Cdouble},
                     Int64, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Int32}),
                    ds.h, nb, J, A, B, c, d, c isa Vector ? 1 : 0, p(ν), length(τ), τ, out, status))
    end
    return out, status
end

"""
    rand_posterior(ds, A, B, c, d, τ, q_data, q_new, ϵ; μ = nothing, ν = nothing, shift = nothing)

Posterior draws at the times `τ` (any order) for every column of `A`, `B`, in O(N + M) per draw by Matheron's rule
(`pioran_celerite_rand_posterior`): what `rand(posterior(fx, y), τ, 1)` (src/scalable_GP.jl:106-112) draws from the dense mean and covariance,
also where `τ` repeats or meets a data time.  `q_data` (`N × nbatch`), `q_new` (`length(τ) × nbatch`), `ϵ` (`N × nbatch`): standard normals of the
latent process at the data times, at `τ`, and of the measurement noise.  `shift`: the shifted log-flux models (the data set holds raw flux and
`yerr.^2`; the draws are in the transformed scale).  Returns the `length(τ) × nbatch` matrix and the status vector (2 and NaN where a draw's
factorisation is not positive definite or `y .- shift` is not positive).
"""
function rand_posterior(ds::Dataset, A::Matrix{Float64}, B::Matrix{Float64}, c::VecOrMat{Float64}, d::VecOrMat{Float64},
                        τ::Vector{Float64}, q_data::Matrix{Float64}, q_new::Matrix{Float64}, ϵ::Matrix{Float64};
                        μ::Union{Nothing, Vector{Float64}} = nothing, ν::Union{Nothing, Vector{Float64}} = nothing,
                        shift::Union{Nothing, Vector{Float64}} = nothing)
    J, nb = size(A)
    size(q_new) == (length(τ), nb) || error("q_new must be length(τ) × nbatch")
    size(q_data) == size(ϵ) && size(q_data, 2) == nb || error("q_data and ϵ must be N × nbatch")
    out = Matrix{Float64}(undef, length(τ), nb)      # column-major = the ABI's [B][M]
    status = zeros(Int32, nb)
    p(x) = x === nothing ? Ptr{Cdouble}(C_NULL) : pointer(x)
    GC.@preserve A B c d μ ν shift τ q_data q_new ϵ out status begin
        check(ccall((:pioran_celerite_rand_posterior, LIB), Cint,
                    (Ptr{Cvoid}, Int64, Int64, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Ptr{Cdouble}, Ptr{Cdouble},
                     Ptr{Cdouble}, Int64, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Int32}),
                    ds.h, nb, J, A, B, c, d, c isa Vector ? 1 : 0, p(μ), p(ν), p(shift), length(τ), τ, q_data, q_new, ϵ, out, status))
    end
    return out, status
end

# Float64 drop-in for Pioran.pred (predict(cov, τ, t, y, σ²) reaches it for every covariance type, :348-361)
function pred_hip(a::Vector{Float64}, b::Vector{Float64}, c::Vector{Float64}, d::Vector{Float64}, τ::Vector{Float64},
                  t::Vector{Float64}, y::Vector{Float64}, σ²::Vector{Float64}; ctx = default_context())
    ds = Dataset(t, y, σ²; ctx = ctx)
    try
        out, _ = predict_batch(ds, reshape(a, :, 1), reshape(b, :, 1), c, d, τ)
        return vec(out)
    finally
        close!(ds)          # release the device copy now, not at the next GC
    end
end

"""
    simulate_batch(A, B, c, d, t, σ², q)

GP realisations `y = L D^(1/2) q` for every column of `A`, `B` (`c`, `d` shared vectors or `J × nbatch` matrices) from the standard
normals `q` (`length(t) × nbatch`);
`simulate(rng, cov, t, σ²)` (src/celerite_solver.jl:497-513) is `simulate_batch(..., randn(rng, N, 1))`.
"""
function simulate_batch(A::Matrix{Float64}, B::Matrix{Float64}, c::VecOrMat{Float64}, d::VecOrMat{Float64}, t::Vector{Float64},
                        σ²::Vector{Float64}, q::Matrix{Float64}; ctx = default_context())
    J, nb = size(A)
    size(q) == (length(t), nb) || error("q must be length(t) × nbatch")
    out = Matrix{Float64}(undef, length(t), nb)
    GC.@preserve A B c d t σ² q out begin
        check(ccall((:pioran_celerite_simulate, LIB), Cint,
                    (Ptr{Cvoid}, Int64, Int64, Int64, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Ptr{Cdouble},
                     Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}),
                    ctx.h, length(t), nb, J, A, B, c, d, c isa Vector ? 1 : 0, t, σ², q, out))
    end
    return out
end

"""
    lombscargle_batch(t, Y, yerr, freq; fit_mean = true, center_data = true)

Generalised Lomb-Scargle power (standard normalisation) of every column of `Y` (`length(t) × nbatch`) at the frequencies `freq` (cycles per
unit time), weights `yerr.^-2` (`yerr = nothing`: equal weights) — `freqpower(lombscargle(t, Y[:, k], yerr, frequencies = freq))[2]` of
LombScargle.jl for all `k` in one call, the loop of `plot_lsp_ppc` (src/plots_diagnostics.jl:532-546).  Returns `(power, status)`:
`power` is `length(freq) × nbatch`; `status[k] == 2` marks a constant or non-finite series (its column is NaN).
"""
function lombscargle_batch(t::Vector{Float64}, Y::Matrix{Float64}, yerr::Union{Nothing, Vector{Float64}}, freq::Vector{Float64};
                           fit_mean::Bool = true, center_data::Bool = true, ctx = default_context())
    N, nb = size(Y)
    N == length(t) || error("Y must be length(t) × nbatch")
    yerr === nothing || length(yerr) == N || error("yerr must have the length of t")
    power = Matrix{Float64}(undef, length(freq), nb)
    status = Vector{Int32}(undef, nb)
    GC.@preserve t Y yerr freq power status begin
        check(ccall((:pioran_lombscargle_batch, LIB), Cint,
                    (Ptr{Cvoid}, Int64, Int64, Int64, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Cint, Ptr{Cdouble},
                     Ptr{Int32}),
                    ctx.h, N, nb, length(freq), t, Y, yerr === nothing ? Ptr{Cdouble}(C_NULL) : pointer(yerr), freq, fit_mean ? 1 : 0,
                    center_data ? 1 : 0, power, status))
    end
    return power, status
end

const PPC_QUANTILES = [0.025, 0.16, 0.5, 0.84, 0.975]

"""
    quantiles_batch(X, probs = PPC_QUANTILES; status, shift, cols, ref, scale)

`[quantile(k, p) for k in eachrow(X), p in probs]` and `mean(X, dims = 2)` of the predictive checks (src/plots_diagnostics.jl:805-816) on the
device: `X` is `M × nbatch`, one draw per column (the reference's `ts_array`).  `status` (`nbatch`): draws with a non-zero entry are left out;
`shift` (`nbatch`): the values are `exp.(X .+ shift')`; `cols` (1-based row indices of `X`, any order): the rows to reduce; `ref`, `scale`
(`length(cols)`): the values are `(ref .- v) ./ scale`.  Returns `(quant, mean, kept)`: `quant` is `Mc × length(probs)`.
"""
function quantiles_batch(X::Matrix{Float64}, probs::Vector{Float64} = PPC_QUANTILES; status::Union{Nothing, Vector{Int32}} = nothing,
                         shift::Union{Nothing, Vector{Float64}} = nothing, cols::Union{Nothing, Vector{<:Integer}} = nothing,
                         ref::Union{Nothing, Vector{Float64}} = nothing, scale::Union{Nothing, Vector{Float64}} = nothing, ctx = default_context())
    M, nb = size(X)
    cols0 = cols === nothing ? nothing : Int32.(cols .- 1)
    Mc = cols0 === nothing ? M : length(cols0)
    quant = Matrix{Float64}(undef, Mc, length(probs))      # column-major = the ABI's [Q][Mc]
    mean = Vector{Float64}(undef, Mc)
    kept = Ref{Int32}(-1)
    p(x) = x === nothing ? Ptr{Cdouble}(C_NULL) : pointer(x)
    pint(x) = x === nothing ? Ptr{Int32}(C_NULL) : pointer(x)
    GC.@preserve X probs status shift cols0 ref scale quant mean begin
        check(ccall((:pioran_quantiles_batch, LIB), Cint,
                    (Ptr{Cvoid}, Int64, Int64, Int64, Ptr{Cdouble}, Ptr{Int32}, Ptr{Cdouble}, Int64, Ptr{Int32}, Ptr{Cdouble}, Ptr{Cdouble},
                     Int64, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ref{Int32}),
                    ctx.h, nb, M, M, X, pint(status), p(shift), Mc, pint(cols0), p(ref), p(scale), length(probs), probs, quant, mean, kept))
    end
    return quant, mean, Int(kept[])
end

"""
    quantiles_batch_dev(ctx, B, M, ldx, dX, probs; dstatus, dshift, Mc, dcols, dref, dscale, dquant, dmean, dkept)

The same on arrays already in device memory (`Ptr`s into HBM; `probs` on the host), asynchronous on the context's stream.
"""
function quantiles_batch_dev(ctx, B::Integer, M::Integer, ldx::Integer, dX::Ptr{Cdouble}, probs::Vector{Float64}; dstatus = Ptr{Int32}(C_NULL),
                             dshift = Ptr{Cdouble}(C_NULL), Mc::Integer = 0, dcols = Ptr{Int32}(C_NULL), dref = Ptr{Cdouble}(C_NULL),
                             dscale = Ptr{Cdouble}(C_NULL), dquant::Ptr{Cdouble}, dmean = Ptr{Cdouble}(C_NULL), dkept = Ptr{Int32}(C_NULL))
    GC.@preserve probs begin
        check(ccall((:pioran_quantiles_batch_dev, LIB), Cint,
                    (Ptr{Cvoid}, Int64, Int64, Int64, Ptr{Cdouble}, Ptr{Int32}, Ptr{Cdouble}, Int64, Ptr{Int32}, Ptr{Cdouble}, Ptr{Cdouble},
                     Int64, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Int32}),
                    ctx.h, B, M, ldx, dX, dstatus, dshift, Mc, dcols, dref, dscale, length(probs), probs, dquant, dmean, dkept))
    end
    return nothing
end

_psd_check_ids(model::Symbol, basis::String) =
    (model === :SingleBendingPowerLaw ? 0 : model === :DoubleBendingPowerLaw ? 1 : error("model $model not supported on the device"),
     basis == "SHO" ? 0 : basis == "DRWCelerite" ? 1 : error("basis $basis not supported on the device"))

"""
    psd_check_batch(model, samples, norm_samples, f, f_min, f_max, n_components; basis_function, S_low, S_high, is_integrated_power,
                    normalise, times_f)

The PSD model and its basis-function approximation for every column of `samples` (`P_params × nbatch`, as the reference passes them) at the
frequencies `f`: `(psd, psd_approx, residuals, ratios, amplitudes, integ, status)` with the four arrays `length(f) × nbatch` as
`sample_approx_model` returns them (src/plots_diagnostics.jl:195-213), `amplitudes` `n_components × nbatch` (`get_approx_coefficients`), `integ`
(`get_norm_psd`) and `status[k] == 2` for a draw that cannot be evaluated (its columns are NaN).  `normalise`: both spectra divided by `integ` as
`plot_psd_ppc` does (:404-409); `times_f`: multiplied by `f` after that (`plot_f_P`).  Continuum models only.
"""
function psd_check_batch(model::Symbol, samples::Matrix{Float64}, norm_samples::Vector{Float64}, f::Vector{Float64}, f_min::Real, f_max::Real,
                         n_components::Integer = 20; basis_function::String = "SHO", S_low::Real = 20.0, S_high::Real = 20.0,
                         is_integrated_power::Bool = true, normalise::Bool = false, times_f::Bool = false, ctx = default_context())
    m, bs = _psd_check_ids(model, basis_function)
    size(samples, 1) == (m == 0 ? 3 : 5) || error("samples must be $(m == 0 ? 3 : 5) × nbatch")
    nb, F = size(samples, 2), length(f)
    length(norm_samples) == nb || error("norm_samples must have one entry per draw")
    psd, psd_approx, residuals, ratios = (Matrix{Float64}(undef, F, nb) for _ in 1:4)
    amplitudes = Matrix{Float64}(undef, n_components, nb); integ = Vector{Float64}(undef, nb); status = Vector{Int32}(undef, nb)
    GC.@preserve samples norm_samples f psd psd_approx residuals ratios amplitudes integ status begin
        check(ccall((:pioran_psd_check_batch, LIB), Cint,
                    (Ptr{Cvoid}, Int64, Cint, Int64, Cint, Cint, Cdouble, Cdouble, Cdouble, Cdouble, Ptr{Cdouble}, Ptr{Cdouble}, Int64,
                     Ptr{Cdouble}, Cint, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Int32}),
                    ctx.h, nb, m, n_components, bs, is_integrated_power ? 1 : 0, f_min, f_max, S_low, S_high, samples, norm_samples, F, f,
                    normalise ? 1 : 0, times_f ? 1 : 0, psd, psd_approx, residuals, ratios, amplitudes, integ, status))
    end
    return psd, psd_approx, residuals, ratios, amplitudes, integ, status
end

"""
    psd_check_batch_dev(ctx, B, model, n_components, dθ, dnorm, F, dfreq, f_min, f_max; dpsd, dpsd_approx, dresiduals, dratios, ...)

The same on arrays already in device memory (`Ptr`s into HBM; any output may be `C_NULL`, not all), asynchronous on the context's stream.
"""
function psd_check_batch_dev(ctx, B::Integer, model::Symbol, n_components::Integer, dθ::Ptr{Cdouble}, dnorm::Ptr{Cdouble}, F::Integer,
                             dfreq::Ptr{Cdouble}, f_min::Real, f_max::Real; basis_function::String = "SHO", S_low::Real = 20.0,
                             S_high::Real = 20.0, is_integrated_power::Bool = true, normalise::Bool = false, times_f::Bool = false,
                             dpsd = Ptr{Cdouble}(C_NULL), dpsd_approx = Ptr{Cdouble}(C_NULL), dresiduals = Ptr{Cdouble}(C_NULL),
                             dratios = Ptr{Cdouble}(C_NULL), damplitudes = Ptr{Cdouble}(C_NULL), dinteg = Ptr{Cdouble}(C_NULL),
                             dstatus = Ptr{Int32}(C_NULL))
    m, bs = _psd_check_ids(model, basis_function)
    check(ccall((:pioran_psd_check_batch_dev, LIB), Cint,
                (Ptr{Cvoid}, Int64, Cint, Int64, Cint, Cint, Cdouble, Cdouble, Cdouble, Cdouble, Ptr{Cdouble}, Ptr{Cdouble}, Int64,
                 Ptr{Cdouble}, Cint, Cint, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Int32}),
                ctx.h, B, m, n_components, bs, is_integrated_power ? 1 : 0, f_min, f_max, S_low, S_high, dθ, dnorm, F, dfreq,
                normalise ? 1 : 0, times_f ? 1 : 0, dpsd, dpsd_approx, dresiduals, dratios, damplitudes, dinteg, dstatus))
    return nothing
end

"""
    psd_check_summary(model, samples, norm_samples, f, f_min, f_max, n_components, probs = PPC_QUANTILES; ...)

`psd_check_batch` with the arrays left on the device and reduced there: `(quant, mean, meta, status, kept)` with `quant` `length(f) × length(probs) × 4`
and `mean` `length(f) × 4` over the draws with status 0 (the last index: psd, psd_approx, residuals, ratios), and `meta` `8 × nbatch`: per draw,
over the frequencies, mean, median, min |·|, max |·| of the residuals, then of the ratios (plot_boxplot_psd_approx, src/plots_diagnostics.jl:43-51).
At most 4096 draws and 4096 frequencies.
"""
function psd_check_summary(model::Symbol, samples::Matrix{Float64}, norm_samples::Vector{Float64}, f::Vector{Float64}, f_min::Real, f_max::Real,
                           n_components::Integer = 20, probs::Vector{Float64} = PPC_QUANTILES; basis_function::String = "SHO", S_low::Real = 20.0,
                           S_high::Real = 20.0, is_integrated_power::Bool = true, normalise::Bool = false, times_f::Bool = false,
                           ctx = default_context())
    m, bs = _psd_check_ids(model, basis_function)
    size(samples, 1) == (m == 0 ? 3 : 5) || error("samples must be $(m == 0 ? 3 : 5) × nbatch")
    nb, F, Q = size(samples, 2), length(f), length(probs)
    length(norm_samples) == nb || error("norm_samples must have one entry per draw")
    quant = Array{Float64, 3}(undef, F, Q, 4); mean = Matrix{Float64}(undef, F, 4); meta = Matrix{Float64}(undef, 8, nb)
    status = Vector{Int32}(undef, nb); kept = Ref{Int32}(-1)
    GC.@preserve samples norm_samples f probs quant mean meta status begin
        check(ccall((:pioran_psd_check_summary, LIB), Cint,
                    (Ptr{Cvoid}, Int64, Cint, Int64, Cint, Cint, Cdouble, Cdouble, Cdouble, Cdouble, Ptr{Cdouble}, Ptr{Cdouble}, Int64,
                     Ptr{Cdouble}, Cint, Cint, Int64, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Int32}, Ref{Int32}),
                    ctx.h, nb, m, n_components, bs, is_integrated_power ? 1 : 0, f_min, f_max, S_low, S_high, samples, norm_samples, F, f,
                    normalise ? 1 : 0, times_f ? 1 : 0, Q, probs, quant, mean, meta, status, kept))
    end
    return quant, mean, meta, status, Int(kept[])
end

"""
    sample_approx_model(samples, norm_samples, f0, fM, model; n_frequencies = 1000, basis_function = "SHO", n_components = 20)

`sample_approx_model` of src/plots_diagnostics.jl:195-213 in one device call: `(psd, psd_approx, residuals, ratios, f)`, the arrays
`n_frequencies × nbatch`.  `model` is `:SingleBendingPowerLaw` or `:DoubleBendingPowerLaw`.
"""
function sample_approx_model(samples::Matrix{Float64}, norm_samples::Vector{Float64}, f0::Real, fM::Real, model::Symbol; n_frequencies::Integer = 1000,
                             basis_function::String = "SHO", n_components::Integer = 20, ctx = default_context())
    f = collect(10 .^ range(log10(f0), log10(fM), n_frequencies))
    psd, psd_approx, residuals, ratios, _, _, _ = psd_check_batch(model, samples, norm_samples, f, f0, fM, n_components;
                                                                  basis_function = basis_function, S_low = 1.0, S_high = 1.0, ctx = ctx)
    return psd, psd_approx, residuals, ratios, f
end

"""
    run_diagnostics(prior_samples, norm_samples, f_min, f_max, model, S_low = 20.0, S_high = 20.0; basis_function = "SHO", n_components = 20)

The numbers of `run_diagnostics` (src/plots_diagnostics.jl:232-240), what its three text files hold: a named tuple with `f`, `mean_res`, `mean_rat`,
`res_quantiles`, `rat_quantiles` (`length(f) × 5`, at `PPC_QUANTILES`), `meta` (`8 × nbatch`: meta_mean, meta_median, meta_min, meta_max, then the
same of the ratios) and `kept`.  One device call; at most 4096 draws (with more, reduce the arrays of `sample_approx_model` on the host).
"""
function run_diagnostics(prior_samples::Matrix{Float64}, norm_samples::Vector{Float64}, f_min::Real, f_max::Real, model::Symbol, S_low::Real = 20.0,
                         S_high::Real = 20.0; basis_function::String = "SHO", n_components::Integer = 20, n_frequencies::Integer = 1000,
                         ctx = default_context())
    f0, fM = f_min / S_low, f_max * S_high
    f = collect(10 .^ range(log10(f0), log10(fM), n_frequencies))
    quant, mean, meta, _, kept = psd_check_summary(model, prior_samples, norm_samples, f, f0, fM, n_components; basis_function = basis_function,
                                                   S_low = 1.0, S_high = 1.0, ctx = ctx)
    return (f = f, mean_res = mean[:, 3], mean_rat = mean[:, 4], res_quantiles = quant[:, :, 3], rat_quantiles = quant[:, :, 4], meta = meta,
            kept = kept)
end

"""
    rand_posterior_summary(ds, A, B, c, d, τ, q_data, q_new, ϵ, probs = PPC_QUANTILES; μ, ν, shift, backtransform, res_cols, res_ref, res_scale)

`rand_posterior_batch` with the draws left on the device and reduced there: quantiles and mean over the draws with status 0 at every `τ`
(`length(τ) × length(probs)`), and, with `res_cols` (1-based indices into `τ`), `res_ref`, `res_scale`, of the residuals
`(res_ref .- draw[res_cols]) ./ res_scale` — the arrays `plot_ppc_timeseries` draws (src/plots_diagnostics.jl:805-816).  `backtransform`
(needs `shift`): summaries of `exp.(draw .+ shift_b)` (:663).  Returns `(ts_quant, ts_mean, res_quant, res_mean, status, kept)`.
"""
function rand_posterior_summary(ds::Dataset, A::Matrix{Float64}, B::Matrix{Float64}, c::VecOrMat{Float64}, d::VecOrMat{Float64},
                                τ::Vector{Float64}, q_data::Matrix{Float64}, q_new::Matrix{Float64}, ϵ::Matrix{Float64},
                                probs::Vector{Float64} = PPC_QUANTILES; μ::Union{Nothing, Vector{Float64}} = nothing,
                                ν::Union{Nothing, Vector{Float64}} = nothing, shift::Union{Nothing, Vector{Float64}} = nothing,
                                backtransform::Bool = false, res_cols::Union{Nothing, Vector{<:Integer}} = nothing,
                                res_ref::Union{Nothing, Vector{Float64}} = nothing, res_scale::Union{Nothing, Vector{Float64}} = nothing)
    J, nb = size(A)
    M, Q = length(τ), length(probs)
    size(q_new) == (M, nb) || error("q_new must be length(τ) × nbatch")
    size(q_data) == size(ϵ) && size(q_data, 2) == nb || error("q_data and ϵ must be N × nbatch")
    cols0 = res_cols === nothing ? nothing : Int32.(res_cols .- 1)
    Nres = cols0 === nothing ? 0 : length(cols0)
    ts_quant = Matrix{Float64}(undef, M, Q); ts_mean = Vector{Float64}(undef, M)
    res_quant = Matrix{Float64}(undef, Nres, Q); res_mean = Vector{Float64}(undef, Nres)
    status = zeros(Int32, nb)
    kept = Ref{Int32}(-1)
    p(x) = x === nothing ? Ptr{Cdouble}(C_NULL) : pointer(x)
    pint(x) = x === nothing ? Ptr{Int32}(C_NULL) : pointer(x)
    GC.@preserve A B c d μ ν shift τ q_data q_new ϵ probs cols0 res_ref res_scale ts_quant ts_mean res_quant res_mean status begin
        check(ccall((:pioran_celerite_rand_posterior_summary, LIB), Cint,
                    (Ptr{Cvoid}, Int64, Int64, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Ptr{Cdouble}, Ptr{Cdouble},
                     Ptr{Cdouble}, Int64, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Int64, Ptr{Cdouble}, Ptr{Cdouble},
                     Ptr{Cdouble}, Int64, Ptr{Int32}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Int32}, Ref{Int32}),
                    ds.h, nb, J, A, B, c, d, c isa Vector ? 1 : 0, p(μ), p(ν), p(shift), M, τ, q_data, q_new, ϵ, backtransform ? 1 : 0, Q, probs,
                    ts_quant, ts_mean, Nres, pint(cols0), p(res_ref), p(res_scale), res_quant, res_mean, status, kept))
    end
    return ts_quant, ts_mean, res_quant, res_mean, status, Int(kept[])
end

# ---- value and gradient (reverse mode through the recurrence on the GPU) --------------------------------------------------
"""
    logpdf_grad_batch(ds, A, B, c, d; μ, ν, series = false, cd = true)

log L and ∂log L/∂(a_j, b_j, c_j, d_j) (`J × nbatch` each), ∂/∂ν, ∂/∂μ for every draw; with `series = true` also ∂/∂y_n and
∂/∂σ²_n (`N × nbatch`).  `cd = false` leaves out ∂/∂(c_j, d_j) — all an `approx`-based model needs, whose `(c, d)` are fixed by the
spectral grid (6.2 instead of 7.0 ms at N = 1e4, J = 20; `grad_c`, `grad_d` are then `nothing`).  `c`, `d`: length-`J` vectors shared by the draws or `J × nbatch` matrices (QPO features, CARMA,
free Celerite terms).  This is what a `ChainRulesCore.rrule` / `LogDensityProblems.logdensity_and_gradient` for the GP
likelihood returns instead of pushing ForwardDiff Duals through `Pioran.logl` (test/test_likelihood.jl:55-60); the chain
rule from (a, b, c, d) to the PSD parameters goes through `approx`, which stays in Julia.
"""
function logpdf_grad_batch(ds::Dataset, A::Matrix{Float64}, B::Matrix{Float64}, c::VecOrMat{Float64}, d::VecOrMat{Float64};
                           μ::Union{Nothing, Vector{Float64}} = nothing, ν::Union{Nothing, Vector{Float64}} = nothing,
                           series::Bool = false, cd::Bool = true)
    J, nb = size(A)
    out = Vector{Float64}(undef, nb); status = zeros(Int32, nb)
    ga = Matrix{Float64}(undef, J, nb); gb = Matrix{Float64}(undef, J, nb)
    gc = cd ? Matrix{Float64}(undef, J, nb) : nothing; gd = cd ? Matrix{Float64}(undef, J, nb) : nothing
    gν = Vector{Float64}(undef, nb); gμ = Vector{Float64}(undef, nb)
    gy = series ? Matrix{Float64}(undef, ds.N, nb) : nothing
    gs = series ? Matrix{Float64}(undef, ds.N, nb) : nothing
    p(x) = x === nothing ? Ptr{Cdouble}(C_NULL) : pointer(x)
    GC.@preserve A B c d μ ν out status ga gb gc gd gν gμ gy gs begin
        check(ccall((:pioran_celerite_logl_grad, LIB), Cint,
                    (Ptr{Cvoid}, Int64, Int64, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Ptr{Cdouble}, Ptr{Cdouble},
                     Ptr{Cdouble}, Ptr{Int32}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble},
                     Ptr{Cdouble}, Ptr{Cdouble}),
                    ds.h, nb, J, A, B, c, d, c isa Vector ? 1 : 0, p(μ), p(ν), out, status, ga, gb, p(gc), p(gd), gν, gμ, p(gy), p(gs)))
    end
    return (logl = out, status = status, grad_a = ga, grad_b = gb, grad_c = gc, grad_d = gd, grad_ν = gν, grad_μ = gμ,
            grad_y = gy, grad_σ² = gs)
end

"""
    logpdf_grad_batch_shift(ds, A, B, c, d, shift; μ, ν)

Value and gradient for the shifted log-flux models (docs/src/turing.md:205-230): `ds` holds the raw flux and `yerr.^2`;
returns in addition `grad_shift` = ∂log L/∂c per draw.
"""
function logpdf_grad_batch_shift(ds::Dataset, A::Matrix{Float64}, B::Matrix{Float64}, c::VecOrMat{Float64}, d::VecOrMat{Float64},
                                 shift::Vector{Float64}; μ::Union{Nothing, Vector{Float64}} = nothing,
                                 ν::Union{Nothing, Vector{Float64}} = nothing)
    J, nb = size(A)
    out = Vector{Float64}(undef, nb); status = zeros(Int32, nb)
    ga = Matrix{Float64}(undef, J, nb); gb = Matrix{Float64}(undef, J, nb)
    gc = Matrix{Float64}(undef, J, nb); gd = Matrix{Float64}(undef, J, nb)
    gν = Vector{Float64}(undef, nb); gμ = Vector{Float64}(undef, nb); gs = Vector{Float64}(undef, nb)
    p(x) = x === nothing ? Ptr{Cdouble}(C_NULL) : pointer(x)
    GC.@preserve A B c d μ ν shift out status ga gb gc gd gν gμ gs begin
        check(ccall((:pioran_celerite_logl_grad_shift, LIB), Cint,
                    (Ptr{Cvoid}, Int64, Int64, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Cint, Ptr{Cdouble}, Ptr{Cdouble},
                     Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Int32}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble},
                     Ptr{Cdouble}, Ptr{Cdouble}),
                    ds.h, nb, J, A, B, c, d, c isa Vector ? 1 : 0, p(μ), p(ν), shift, out, status, ga, gb, gc, gd, gν, gμ, gs))
    end
    return (logl = out, status = status, grad_a = ga, grad_b = gb, grad_c = gc, grad_d = gd, grad_ν = gν, grad_μ = gμ, grad_shift = gs)
end

# ---- dense solver: log_likelihood_direct (src/direct_solver.jl:6-21), returns +NLL -------------------------
function log_likelihood_direct_hip(cov::SemiSeparable, t::Vector{Float64}, y::Vector{Float64}, σ²::Vector{Float64};
                                   ctx = default_context())
    a, b, c, d = map(v -> collect(Float64, real.(v)), celerite_coefs(cov))
    out = Ref{Cdouble}(NaN)
    info = Ref{Int32}(0)
    GC.@preserve a b c d t y σ² check(ccall((:pioran_dense_nll, LIB), Cint,
        (Ptr{Cvoid}, Int64, Int64, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble},
         Ptr{Cdouble}, Ref{Cdouble}, Ref{Int32}), ctx.h, length(t), length(a), a, b, c, d, t, y, σ², out, info))
    info[] != 0 && throw(LinearAlgebra.PosDefException(info[]))
    return out[]
end

# predict_cov (src/direct_solver.jl:28-69): posterior covariance at τ, the matrix behind cov / std / rand of a PosteriorGP
function predict_cov_hip(cov::SemiSeparable, τ::Vector{Float64}, t::Vector{Float64}, σ²::Vector{Float64}; ctx = default_context())
    a, b, c, d = map(v -> collect(Float64, real.(v)), celerite_coefs(cov))
    M = length(τ)
    out = Matrix{Float64}(undef, M, M)
    info = Ref{Int32}(0)
    GC.@preserve a b c d τ t σ² out check(ccall((:pioran_dense_predict_cov, LIB), Cint,
        (Ptr{Cvoid}, Int64, Int64, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Int64,
         Ptr{Cdouble}, Ptr{Cdouble}, Ref{Int32}), ctx.h, length(t), length(a), a, b, c, d, t, σ², M, τ, out, info))
    info[] != 0 && throw(LinearAlgebra.PosDefException(info[]))
    return out
end

# predict_direct (src/direct_solver.jl:75-119): dense posterior mean (and covariance) — the reference's ground truth for `predict`
function predict_direct_hip(cov::SemiSeparable, τ::Vector{Float64}, t::Vector{Float64}, y::Vector{Float64}, σ²::Vector{Float64},
                            with_covariance::Bool = false; ctx = default_context())
    a, b, c, d = map(v -> collect(Float64, real.(v)), celerite_coefs(cov))
    M = length(τ)
    μ = Vector{Float64}(undef, M)
    K = with_covariance ? Matrix{Float64}(undef, M, M) : nothing
    info = Ref{Int32}(0)
    GC.@preserve a b c d τ t y σ² μ K check(ccall((:pioran_dense_predict, LIB), Cint,
        (Ptr{Cvoid}, Int64, Int64, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble},
         Int64, Ptr{Cdouble}, Ptr{Cdouble}, Ptr{Cdouble}, Ref{Int32}), ctx.h, length(t), length(a), a, b, c, d, t, y, σ², M, τ, μ,
        K === nothing ? Ptr{Cdouble}(C_NULL) : pointer(K), info))
    info[] != 0 && throw(LinearAlgebra.PosDefException(info[]))
    return with_covariance ? (μ, K) : μ
end

"""
    step_route(family, R; standard_rows=0, n_complex=0, B=1, shared_table=true, npd_rows=0, per_draw_tables=false, options="")

Diagnostics (no GPU needed): the kernel instantiation a step-by-step launch runs (`pioran_step_route`) — `family = "scan"` for the throughput
layout, `"value"`, `"store"`, `"simulate"` or `"gradient"` for the latency layout's modes.  Returns `(name, plan)`: the name
`pioran_celerite_config_name(0)` reports after such a launch (`nothing` where the family refuses) and the plan's eight integers
(`include/pioran_hip.h`).
"""
function step_route(family::AbstractString, R::Integer; standard_rows::Integer=0, n_complex::Integer=0, B::Integer=1, shared_table::Bool=true,
                    npd_rows::Integer=0, per_draw_tables::Bool=false, options::AbstractString="")
    name = zeros(UInt8, 64)
    plan = zeros(Int32, 8)
    rc = ccall((:pioran_step_route, LIB), Cint,
               (Cstring, Int32, Int32, Int32, Int64, Cint, Int32, Cint, Cstring, Ptr{UInt8}, Cint, Ptr{Int32}),
               family, R, standard_rows, n_complex, B, shared_table, npd_rows, per_draw_tables, options, name, length(name), plan)
    rc == -4 && return (nothing, plan)
    check(rc)
    return (GC.@preserve(name, unsafe_string(pointer(name))), plan)
end

"""
    window_route(family; R=0, J=0, B=1, npd_rows=0, per_draw_series=false, want_cd=false, tp_rows=0, tp_segments=0, tp_mode=0, options="")

Diagnostics (no GPU needed): the kernel instantiations a launch of the windowed kernels (`family = "block"`, `"block_grad"`, `"block_solve"`,
`"block_sim"`), of their one-draw-per-wavefront form (`"tile"`, `"tile_grad"`) or of the time-parallel family (`"tp"`) runs
(`pioran_window_route`).  Returns `(name, plan)`: the name `pioran_celerite_config_name(-2)` reports after such a launch (`nothing` where it is
refused) and the plan's twelve integers (`include/pioran_hip.h`).
"""
function window_route(family::AbstractString; R::Integer=0, J::Integer=0, B::Integer=1, npd_rows::Integer=0, per_draw_series::Bool=false,
                      want_cd::Bool=false, tp_rows::Integer=0, tp_segments::Integer=0, tp_mode::Integer=0, options::AbstractString="")
    name = zeros(UInt8, 96)
    plan = zeros(Int32, 12)
    rc = ccall((:pioran_window_route, LIB), Cint,
               (Cstring, Int32, Int32, Int64, Int32, Cint, Cint, Int32, Int32, Cint, Cstring, Ptr{UInt8}, Cint, Ptr{Int32}),
               family, R, J, B, npd_rows, per_draw_series, want_cd, tp_rows, tp_segments, tp_mode, options, name, length(name), plan)
    rc == -4 && return (nothing, plan)
    check(rc)
    return (GC.@preserve(name, unsafe_string(pointer(name))), plan)
end

end # module
