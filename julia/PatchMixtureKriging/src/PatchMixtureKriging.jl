# PatchMixtureKriging -- drop-in Julia front end of the MI355X implementation.
#
# Same module name, kernel types and fit/query API as RoyCCWang/PatchMixtureKriging, so that the
# reference's examples/mixGP.jl and examples/IBB1D.jl run unchanged; every numerical method is a
# `ccall` into libpmk_hip.so (C ABI: include/pmk.h).  Set ENV["PMK_LIB"] to the library path
# (default: ../../../patchmixturekriging_amd/csrc/libpmk_hip.so relative to this file).
#
# NOTE: Julia is not installed in the build container, so this file has never been executed there.
# It is kept mechanical and is mirrored 1:1 by the Python package patchmixturekriging_amd, which is
# what the test-suite drives (see INTEGRATION.md).  Indices cross the ABI 0-based; this file adds 1.
module PatchMixtureKriging

using LinearAlgebra
import Libdl

const libpmk = get(ENV, "PMK_LIB",
    normpath(joinpath(@__DIR__, "..", "..", "..", "patchmixturekriging_amd", "csrc", "libpmk_hip.so")))

export RKHSProblemType, fitRKHS!, query!, constructkernelmatrix, evalkernel, evalquery,
       setuppartition, getpartitionlines!, organizetrainingsets, fetchhyperplanes,
       MixtureGPType, MixtureGPDebugType, fitmixtureGP!, fitmixtureGPmulti!, querymixtureGPmulti!,
       logevidencemixtureGP, logevidencemixtureGPmulti, loomixtureGP, loomixtureGPmulti,
       settrendmixtureGP!, trendmixtureGP, trendinfomixtureGP,
       selectmixtureGP!, selectcandidates, loomixtureGP_blend, loomixtureGP_blend_multi, selectblendGP_multi!,
       querymixtureGP_grad, querymixtureGP_vgrad, querymixtureGP_cov, querymixtureGP_cov_multi, querymixtureGP_block, samplemixtureGP_blocks, appendmixtureGP!, capacitymixtureGP,
       removemixtureGP!, removablemixtureGP, reservemixtureGP!

# ------------------------------------------------------------------------------------------ errors
struct PMKError <: Exception
    msg::String
end
lasterror() = unsafe_string(ccall((:pmk_last_error, libpmk), Cstring, ()))
function check(rc::Integer, what::String)
    rc < 0 && throw(PMKError("$what failed ($rc): $(lasterror())"))
    return rc
end

# ------------------------------------------------------------------------------------------ context
const CTX = Ref{Ptr{Cvoid}}(C_NULL)
function context()
    if CTX[] == C_NULL
        h = Ref{Ptr{Cvoid}}(C_NULL)
        dev = parse(Int, get(ENV, "PMK_DEVICE", "0"))
        check(ccall((:pmk_ctx_create, libpmk), Cint, (Cint, Ref{Ptr{Cvoid}}), dev, h), "pmk_ctx_create")
        CTX[] = h[]
    end
    return CTX[]
end

# ------------------------------------------------------------------------------------------ kernel types
# same names and fields as src/misc/declarations.jl:18-111 of the reference
abstract type StationaryKernelType end
abstract type BrownianBridgeKernelType end
struct Spline12KernelType{T} <: StationaryKernelType; a::T; end
struct Spline32KernelType{T} <: StationaryKernelType; a::T; end
struct Spline34KernelType{T} <: StationaryKernelType; a::T; end
struct RationalQuadraticKernelType{T} <: StationaryKernelType; a::T; end
struct TunableRationalQuadraticKernelType{T} <: StationaryKernelType; a::T; w::T; end
struct ModulatedSqExpKernelType{T} <: StationaryKernelType; ϵ_sq::T; ν::T; end
struct GaussianKernel1DType{T} <: StationaryKernelType; ϵ_sq::T; end
struct BrownianBridge10{T} <: BrownianBridgeKernelType; a::T; end
struct BrownianBridge20{T} <: BrownianBridgeKernelType; a::T; end
struct BrownianBridge1ϵ{T} <: BrownianBridgeKernelType; ϵ::T; end
struct BrownianBridge2ϵ{T} <: BrownianBridgeKernelType; ϵ::T; end
struct BrownianBridgeSemiInfDomain{BT <: BrownianBridgeKernelType}; θ_base::BT; end

# pmk_kernel_desc { int32 family; int32 flags; double p[4]; }
struct KernelDesc
    family::Int32
    flags::Int32
    p::NTuple{4,Float64}
end
desc(f, p1 = 0.0, p2 = 0.0; flags = 0) = KernelDesc(Int32(f), Int32(flags), (Float64(p1), Float64(p2), 0.0, 0.0))
desc(θ::Spline34KernelType) = desc(1, θ.a[1])
desc(θ::Spline12KernelType) = desc(2, θ.a[1])
desc(θ::Spline32KernelType) = desc(3, θ.a[1])
desc(θ::GaussianKernel1DType) = desc(4, θ.ϵ_sq[1])
desc(θ::RationalQuadraticKernelType) = desc(5, θ.a[1])
desc(θ::TunableRationalQuadraticKernelType) = desc(6, θ.a[1], θ.w[1])
desc(θ::ModulatedSqExpKernelType) = desc(7, θ.ϵ_sq[1], θ.ν[1])
desc(θ::BrownianBridge10) = desc(10, θ.a)
desc(θ::BrownianBridge20) = desc(11, θ.a)
desc(θ::BrownianBridge1ϵ) = desc(12, θ.ϵ)
desc(θ::BrownianBridge2ϵ) = desc(13, θ.ϵ)
function desc(θ::BrownianBridgeSemiInfDomain)
    d = desc(θ.θ_base)
    return KernelDesc(d.family, Int32(1), d.p)
end

# ------------------------------------------------------------------------------------------ closure-carrying kernels
# src/misc/declarations.jl:113-135, src/RKHS/kernel.jl:31-67,87-139.  A closure cannot cross the C ABI and need not: every
# one of these kernels is a stationary canonical kernel on τ² = |p - q|² + Σᵢ (gᵢ(p) - gᵢ(q))² with gᵢ a weighted warp
# function.  The warp functions are evaluated HERE, once per point (the table the reference's FastAdaptiveKernelType
# keeps as w_X), and appended to the coordinates; the device evaluates the canonical kernel on the augmented points
# (input dimension + number of warps ≤ 4).
struct AdaptiveKernelType{KT}
    canonical_params::KT
    warpfunc::Function
end
struct FastAdaptiveKernelType{KT,T,D}
    canonical_kernel::KT
    warpfuncs::Vector{Function}
    w_X::Array{T,D}      # pre-computed warp map evaluations at the training positions (refreshed by constructkernelmatrix)
    s::Vector{T}
end
struct AdaptiveKernelMultiWarpType{KT,T}
    canonical_params::KT
    warpfuncs::Vector{Function}
    a::Vector{T}
end
# the DPP variants (declarations.jl:115-118, 141-149; kernel.jl:70-89, 102-113): the same warped kernel where p != q, and a
# point-dependent term where p == q (1 + g(p)², resp. 1 + self_gain Σ aₘ |wₘ(p)|) -- on the device a per-point addend of
# the kernel's diagonal (pmk_model_set_diag / pmk_query_set_diag)
struct AdaptiveKernelDPPType{KT}
    canonical_params::KT
    warpfunc::Function
end
struct AdaptiveKernelMultiWarpDPPType{KT,T}
    canonical_params::KT
    warpfuncs::Vector{Function}
    a::Vector{T}
    self_gain::T
end
const DPPKernel = Union{AdaptiveKernelDPPType,AdaptiveKernelMultiWarpDPPType}
const WarpedKernel = Union{AdaptiveKernelType,FastAdaptiveKernelType,AdaptiveKernelMultiWarpType,AdaptiveKernelDPPType,
                           AdaptiveKernelMultiWarpDPPType}
canonical(θ::AdaptiveKernelType) = θ.canonical_params
canonical(θ::FastAdaptiveKernelType) = θ.canonical_kernel
canonical(θ::AdaptiveKernelMultiWarpType) = θ.canonical_params
canonical(θ::AdaptiveKernelDPPType) = θ.canonical_params
canonical(θ::AdaptiveKernelMultiWarpDPPType) = θ.canonical_params
desc(θ::WarpedKernel) = desc(canonical(θ))
features(θ::AdaptiveKernelType, x) = [Float64(θ.warpfunc(x))]
features(θ::AdaptiveKernelDPPType, x) = [Float64(θ.warpfunc(x))]
features(θ::FastAdaptiveKernelType, x) = [Float64(θ.s[i] * θ.warpfuncs[i](x)) for i = 1:length(θ.warpfuncs)]
features(θ::AdaptiveKernelMultiWarpType, x) = [Float64(sqrt(θ.a[m]) * θ.warpfuncs[m](x)) for m = 1:length(θ.warpfuncs)]
features(θ::AdaptiveKernelMultiWarpDPPType, x) = [Float64(sqrt(θ.a[m]) * θ.warpfuncs[m](x)) for m = 1:length(θ.warpfuncs)]
# the diagonal term of a kernel at the points X: nothing for every kernel but the DPP variants
diagaddend(θ, X) = nothing
diagaddend(θ::AdaptiveKernelDPPType, X) = Float64[θ.warpfunc(x)^2 for x in X]
diagaddend(θ::AdaptiveKernelMultiWarpDPPType, X) =
    Float64[θ.self_gain * sum(θ.a[m] * abs(θ.warpfuncs[m](x)) for m = 1:length(θ.warpfuncs)) for x in X]

# ------------------------------------------------------------------------------------------ helpers
"""array2matrix (src/misc/utilities.jl:25-36): Vector{Vector{T}} -> D x N matrix"""
function array2matrix(X::Vector{Vector{T}})::Matrix{T} where T
    N = length(X); D = length(X[1])
    out = Matrix{T}(undef, D, N)
    for n = 1:N
        out[:, n] = X[n]
    end
    return out
end
pack(X::Vector{Vector{T}}) where T = Matrix{Float64}(array2matrix(X))
pack(X::Vector{T}) where T <: Real = reshape(Vector{Float64}(X), 1, length(X))
# the points the device evaluates kernel θ on: X itself, or X with the warp features appended
kpack(θ, X) = pack(X)
function kpack(θ::WarpedKernel, X::Vector{Vector{T}}) where T
    Xa = [vcat(Vector{Float64}(x), features(θ, x)) for x in X]
    length(Xa[1]) <= 4 || throw(PMKError("input dimension + number of warp functions must be <= 4 on the device path"))
    return pack(Xa)
end

"""convert2itpindex (src/misc/utilities.jl:562-579)"""
function convert2itpindex(x::Vector{T}, a::Vector{T}, b::Vector{T}, M::Vector{Int})::Vector{T} where T <: Real
    @assert length(x) == length(a) == length(b)
    return collect((x[d] - a[d]) / (b[d] - a[d]) * (M[d] - 1) + 1 for d = 1:length(x))
end

# ------------------------------------------------------------------------------------------ kernel matrix
"""constructkernelmatrix(X, θ)::Matrix{Float64} (src/RKHS/RKHS.jl:4-34); host matrix, exactly symmetric"""
function constructkernelmatrix(X, θ)::Matrix{Float64}
    if θ isa FastAdaptiveKernelType                     # RKHS.jl:141-146: refresh the warp table
        for i = 1:length(θ.warpfuncs), n = 1:length(X)
            θ.w_X[n, i] = θ.warpfuncs[i](X[n])
        end
    end
    Xm = kpack(θ, X); D, n = size(Xm)
    K = Matrix{Float64}(undef, n, n)
    d = Ref(desc(θ))
    check(ccall((:pmk_kernel_matrix, libpmk), Cint,
        (Ptr{Cvoid}, Ref{KernelDesc}, Cint, Int64, Ptr{Float64}, Int64, Ptr{Float64}, Ptr{Float64}, Int64),
        context(), d, D, n, Xm, n, C_NULL, K, n), "constructkernelmatrix")
    g = diagaddend(θ, X)
    if g !== nothing                                    # kernel.jl:74, 108: where p == q (by distance: duplicates too)
        for i = 1:n, j = 1:i
            if i == j || X[i] == X[j]
                K[i, j] += g[i]
                i == j || (K[j, i] += g[i])
            end
        end
    end
    return K
end
"""constructkernelmatrix(X, Z, θ) (src/RKHS/RKHS.jl:95-110)"""
function constructkernelmatrix(X::Vector{Vector{T}}, Z::Vector{Vector{T}}, θ)::Matrix{T} where T
    Xm = kpack(θ, X); Zm = kpack(θ, Z); D, n = size(Xm); m = size(Zm, 2)
    K = Matrix{Float64}(undef, n, m)
    d = Ref(desc(θ))
    check(ccall((:pmk_kernel_matrix, libpmk), Cint,
        (Ptr{Cvoid}, Ref{KernelDesc}, Cint, Int64, Ptr{Float64}, Int64, Ptr{Float64}, Ptr{Float64}, Int64),
        context(), d, D, n, Xm, m, Zm, K, n), "constructkernelmatrix")
    g = diagaddend(θ, X)
    if g !== nothing
        for i = 1:n, j = 1:m
            X[i] == Z[j] && (K[i, j] += g[i])
        end
    end
    return K
end
evalkernel(p::Vector{T}, q::Vector{T}, θ) where T = constructkernelmatrix([p], [q], θ)[1, 1]
evalkernel(p::T, q::T, θ) where T <: Real = constructkernelmatrix([[p]], [[q]], θ)[1, 1]
evalkernel(τ::T, θ::StationaryKernelType) where T <: Real = evalkernel([τ], [zero(T)], θ)

# ------------------------------------------------------------------------------------------ BSP tree
mutable struct HyperplaneType{T}          # partition.jl:3-9
    v::Vector{T}
    c::T
    HyperplaneType{T}(v, c) where T = new{T}(v, c)
    HyperplaneType{T}() where T = new{T}()
end
mutable struct PartitionDataType{T}       # partition.jl:11-16
    hp::HyperplaneType{T}
    X::Vector{Vector{T}}
    global_X_indices::Vector{Int}
    index::Int
end
mutable struct BinaryNode{T}              # partition.jl:18-29
    data::T
    parent::BinaryNode{T}
    left::BinaryNode{T}
    right::BinaryNode{T}
    BinaryNode{T}(data) where T = new{T}(data)
    BinaryNode{T}(data, parent::BinaryNode{T}) where T = new{T}(data, parent)
end
BinaryNode(data) = BinaryNode{typeof(data)}(data)

# the native tree (pmk_bsp*) of every root returned by setuppartition.  Weak keys: the table must not keep a root
# alive, or its finalizer (which frees the native tree) would never run.
const NATIVE = WeakKeyDict{Any,Ptr{Cvoid}}()
native(root) = get(NATIVE, root) do
    throw(PMKError("this node is not a root returned by setuppartition"))
end

function buildnodes(h::Ptr{Cvoid}, D::Int, levels::Int, X)
    P = Int(ccall((:pmk_bsp_num_leaves, libpmk), Int64, (Ptr{Cvoid},), h))
    N = Int(ccall((:pmk_bsp_num_points, libpmk), Int64, (Ptr{Cvoid},), h))
    hv = Matrix{Float64}(undef, D, P - 1); hc = Vector{Float64}(undef, P - 1)
    off = Vector{Int64}(undef, P + 1); inds = Vector{Int64}(undef, max(N, 1))
    check(ccall((:pmk_bsp_arrays, libpmk), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Ptr{Int64}, Ptr{Int64}),
        h, hv, hc, off, inds), "pmk_bsp_arrays")
    T = Float64
    k = Ref(0); leaf = Ref(0)
    function make(parent, depth)
        if depth == levels - 1
            leaf[] += 1
            gi = N > 0 ? Vector{Int}(inds[off[leaf[]]+1:off[leaf[]+1]] .+ 1) : Int[]
            data = PartitionDataType(HyperplaneType{T}(), Vector{Vector{T}}(undef, 0), gi, leaf[])
            return parent === nothing ? BinaryNode(data) : BinaryNode{typeof(data)}(data, parent)
        end
        k[] += 1
        data = PartitionDataType(HyperplaneType{T}(hv[:, k[]], hc[k[]]), Vector{Vector{T}}(undef, 0), Int[], 0)
        node = parent === nothing ? BinaryNode(data) : BinaryNode{typeof(data)}(data, parent)
        node.left = make(node, depth + 1)       # pre-order: left subtree first
        node.right = make(node, depth + 1)
        return node
    end
    return make(nothing, 0), off, inds
end

"""setuppartition(X, level) -> root, X_parts, X_parts_inds (src/patchwork/partition.jl:106-129);
`device = true` builds the tree on the GPU (pmk_bsp_build_device, same result bit for bit).  `sign_mode` / `dot_mode`
select between the two readings of two Julia-stdlib behaviours the reference's text does not fix (include/pmk.h)."""
function setuppartition(X::Vector{Vector{T}}, level; sign_mode::Int = 1, dot_mode::Int = 0, device::Bool = false) where T
    Xm = pack(X); D, N = size(Xm)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    if device
        check(ccall((:pmk_bsp_build_device, libpmk), Cint,
            (Ptr{Cvoid}, Cint, Int64, Ptr{Float64}, Cint, Cint, Cint, Ref{Ptr{Cvoid}}),
            context(), D, N, Xm, level, sign_mode, dot_mode, h), "setuppartition")
    else
        check(ccall((:pmk_bsp_build, libpmk), Cint, (Cint, Int64, Ptr{Float64}, Cint, Cint, Cint, Ref{Ptr{Cvoid}}),
            D, N, Xm, level, sign_mode, dot_mode, h), "setuppartition")
    end
    root, off, inds = buildnodes(h[], D, Int(level), X)
    NATIVE[root] = h[]
    let hh = h[]
        finalizer(r -> (ccall((:pmk_bsp_destroy, libpmk), Cvoid, (Ptr{Cvoid},), hh); nothing), root)
    end
    P = length(off) - 1
    X_parts_inds = [Vector{Int}(inds[off[l]+1:off[l+1]] .+ 1) for l = 1:P]
    X_parts = [Vector{Vector{Float64}}(X[ix]) for ix in X_parts_inds]      # labelleafnodes, partition.jl:131-159
    return root, X_parts, X_parts_inds
end

"""findpartition(x, root, levels) (partition.jl:248-262), 1-based leaf index"""
findpartition(x::Vector{T}, root, levels::Int) where T =
    Int(ccall((:pmk_bsp_findpartition, libpmk), Int64, (Ptr{Cvoid}, Ptr{Float64}), native(root), Vector{Float64}(x))) + 1

"""organizetrainingsets(root, levels, X0, ε) (partition.jl:301-357); `device = true`: pmk_bsp_assign_device"""
function organizetrainingsets(root, levels::Int, X0::Vector{Vector{T}}, ε::T; device::Bool = false) where T
    Xm = pack(X0); D, N = size(Xm)
    h = native(root)
    P = Int(ccall((:pmk_bsp_num_leaves, libpmk), Int64, (Ptr{Cvoid},), h))
    off = Vector{Int64}(undef, P + 1)
    # (ccall wants its argument types as a literal tuple at every call site)
    assign(o, i, lo, li) = device ?
        ccall((:pmk_bsp_assign_device, libpmk), Cint,
              (Ptr{Cvoid}, Ptr{Cvoid}, Int64, Ptr{Float64}, Float64, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}),
              context(), h, N, Xm, ε, o, i, lo, li) :
        ccall((:pmk_bsp_assign, libpmk), Cint,
              (Ptr{Cvoid}, Int64, Ptr{Float64}, Float64, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}),
              h, N, Xm, ε, o, i, lo, li)
    check(assign(off, C_NULL, C_NULL, C_NULL), "organizetrainingsets")
    inds = Vector{Int64}(undef, max(off[end], 1)); loff = Vector{Int64}(undef, N + 1); lists = similar(inds)
    check(assign(off, inds, loff, lists), "organizetrainingsets")
    X_set_inds = [Vector{Int}(inds[off[r]+1:off[r+1]] .+ 1) for r = 1:P]
    X_set = [X0[ix] for ix in X_set_inds]
    regions_list_set = [Vector{Int}(lists[loff[n]+1:loff[n+1]] .+ 1) for n = 1:N]
    problematic_inds = Vector{Vector{Int}}(undef, 0)
    return X_set, X_set_inds, regions_list_set, problematic_inds
end

"""fetchhyperplanes(root): pre-order (src/RKHS/mixtureGP.jl:322-334)"""
function fetchhyperplanes(root::BinaryNode{PartitionDataType{T}}) where T
    hps = Vector{HyperplaneType{T}}(undef, 0)
    function visit(node)
        isdefined(node.data.hp, :v) && push!(hps, node.data.hp)
        isdefined(node, :left) && visit(node.left)
        isdefined(node, :right) && visit(node.right)
    end
    visit(root)
    return hps
end

"""findneighbourpartitions(p, radius, root, levels, hps, home; δ) (mixtureGP.jl:339-405)"""
function findneighbourpartitions(p::Vector{T}, radius::T, root, levels, hps, p_region_ind::Int; δ::T = 1e-10) where T
    h = native(root); D = length(p); M = length(hps)
    reg = Vector{Int64}(undef, max(M, 1)); ts = Vector{Float64}(undef, M); zs = Matrix{Float64}(undef, D, M)
    keep = Vector{UInt8}(undef, M)
    k = ccall((:pmk_bsp_neighbours, libpmk), Int64,
        (Ptr{Cvoid}, Ptr{Float64}, Float64, Float64, Int64, Ptr{Int64}, Ptr{Float64}, Ptr{Float64}, Ptr{UInt8}),
        h, Vector{Float64}(p), radius, δ, p_region_ind - 1, reg, ts, zs, keep)
    check(k, "findneighbourpartitions")
    return Vector{Int}(reg[1:k] .+ 1), ts, [zs[:, i] for i = 1:M], BitVector(keep .!= 0)
end

# plotting helpers of src/patchwork/visualize_2D.jl (host only)
function get2Dline(u::Vector{T}, c::T) where T
    return -u[1] / u[2], c / u[2]
end
function prunepartitionline(node, y::Vector{T}, t::Vector{T}) where T
    @assert length(y) == length(t)
    isdefined(node, :parent) || return y, t
    c = node.parent.data.hp.c; v = node.parent.data.hp.v
    isright = node.parent.right === node
    keep = [xor(dot(v, [t[n]; y[n]]) < c, isright) for n = 1:length(t)]
    return prunepartitionline(node.parent, y[keep], t[keep])
end
function getpartitionlines!(y_set::Vector{Vector{T}}, t_set, node::BinaryNode{PartitionDataType{T}}, level::Int,
                            min_t, max_t, max_N_t::Int, centroid::Vector{T}, max_dist::T) where T
    m, b = get2Dline(node.data.hp.v, node.data.hp.c)
    t = collect(LinRange(min_t, max_t, max_N_t)); y = m .* t .+ b
    near = [norm([t[n]; y[n]] - centroid) < max_dist for n = 1:length(t)]
    y_pruned, t_pruned = prunepartitionline(node, y[near], t[near])
    push!(y_set, y_pruned); push!(t_set, t_pruned)
    if level != 2
        getpartitionlines!(y_set, t_set, node.left, level - 1, min_t, max_t, max_N_t, centroid, max_dist)
        getpartitionlines!(y_set, t_set, node.right, level - 1, min_t, max_t, max_N_t, centroid, max_dist)
    end
    return nothing
end

# ------------------------------------------------------------------------------------------ mixture GP
mutable struct MixtureGPDebugType{T}      # mixtureGP.jl:5-35
    w_tilde_set::Vector{Vector{T}}; u_set::Vector{Vector{T}}; v_set::Vector{Vector{T}}
    region_inds_set::Vector{Vector{Int}}; p_region_ind_set::Vector{Int}
    hps_keep_flags_set::Vector{BitVector}; zs_set::Vector{Vector{Vector{T}}}; ts_set::Vector{Vector{T}}
end
MixtureGPDebugType(dummy_val::T) where T = MixtureGPDebugType{T}([], [], [], [], [], [], [], [])

"""U_set / L_set of a fitted model (mixtureGP.jl:43-46): the factors stay on the device (2 x 8 n² bytes per patch, 16.8 GB
at 256 x 2000) and `η.L_set[r]` / `η.U_set[r]` pull ONE patch to the host on first use and keep it, as the Python mirror
does (mixture.py, _LazyFactors).  Indexes and iterates like the reference's Vector."""
mutable struct LazyFactors{T,M} <: AbstractVector{M}
    model::Ref{Ptr{Cvoid}}      # shared with the MixtureGPType that owns the device model
    what::Int                   # pmk_model_get selector: 1 = L (chol_U.L), 2 = K without noise (U_set)
    n::Vector{Int}
    cache::Dict{Int,M}
end
Base.size(f::LazyFactors) = (length(f.n),)
Base.IndexStyle(::Type{<:LazyFactors}) = IndexLinear()
function Base.getindex(f::LazyFactors{T,M}, r::Int) where {T,M}
    haskey(f.cache, r) && return f.cache[r]
    f.model[] == C_NULL && throw(PMKError("fitmixtureGP! must run before U_set / L_set are read"))
    A = Matrix{T}(model_get(f.model[], r, f.what, f.n[r]))
    f.cache[r] = f.what == 1 ? LowerTriangular(A) : A          # exactly M in either case
    return f.cache[r]
end
Base.setindex!(f::LazyFactors, v, r::Int) = (f.cache[r] = v)

mutable struct MixtureGPType{T}           # mixtureGP.jl:38-52 (+ the device model handle)
    X_parts::Vector{Vector{Vector{T}}}
    c_set::Vector{Vector{T}}
    σ²_set::Vector{T}
    U_set::LazyFactors{T,Matrix{T}}
    L_set::LazyFactors{T,LowerTriangular{T,Matrix{T}}}
    hps::Vector{HyperplaneType{T}}
    model::Ptr{Cvoid}
    handle::Ref{Ptr{Cvoid}}     # the same handle, shared with U_set / L_set
    θ_set::Vector{Any}          # the kernel of every patch after fitmixtureGP!(η, y_parts, θs, σ²s); empty otherwise
    N_global::Int               # > 0: built by MixtureGPType(root, X, ε) from N_global points; the model is resident
    R_multi::Int                # target columns the model holds (fitmixtureGPmulti!): the library writes this many, so the
                                # wrappers that size output arrays from a caller's R refuse any other value
end
function MixtureGPType(X_parts::Vector{Vector{Vector{T}}}, hps::Vector{HyperplaneType{T}}) where T
    N = length(X_parts)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    n = Int[length(X) for X in X_parts]
    η = MixtureGPType{T}(X_parts, Vector{Vector{T}}(undef, N), Vector{T}(undef, N),
                         LazyFactors{T,Matrix{T}}(h, 2, n, Dict{Int,Matrix{T}}()),
                         LazyFactors{T,LowerTriangular{T,Matrix{T}}}(h, 1, n, Dict{Int,LowerTriangular{T,Matrix{T}}}()),
                         hps, C_NULL, h, Any[], 0, 0)
    finalizer(e -> (e.model != C_NULL && ccall((:pmk_model_destroy, libpmk), Cvoid, (Ptr{Cvoid},), e.model); nothing), η)
    return η
end

"""MixtureGPType(root, X, ε) -> η: the patches of the tree `root` from ONE global point matrix X (D x N), assigned, gathered
and packed on the device (pmk_model_create_from_bsp).  ε >= 0: the ε-sets of organizetrainingsets; ε < 0: the tree's own
leaves (setuppartition; X must be the matrix the tree was built on).  The tree is attached and the model stays resident:
fitmixtureGP!(η, y::Vector, θ, σ²) takes the targets of all N points.  Kernels that carry a closure are refused there:
their points carry more coordinates than the tree."""
function MixtureGPType(root, X::Matrix{Float64}, ε::Real)
    N = size(X, 2)
    h = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:pmk_model_create_from_bsp, libpmk), Cint,
        (Ptr{Cvoid}, Ptr{Cvoid}, Int64, Ptr{Float64}, Ptr{Float64}, Float64, Int64, Int64, Cint, Ref{Ptr{Cvoid}}),
        context(), native(root), N, X, C_NULL, Float64(ε), 0, 0, 0, h), "pmk_model_create_from_bsp")
    P = Int(ccall((:pmk_model_num_patches, libpmk), Int64, (Ptr{Cvoid},), h[]))
    off = Vector{Int64}(undef, P + 1)
    check(ccall((:pmk_model_patch_index, libpmk), Cint, (Ptr{Cvoid}, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}), h[], C_NULL, off, C_NULL),
          "pmk_model_patch_index")
    inds = Vector{Int64}(undef, max(off[end], 1))
    check(ccall((:pmk_model_patch_index, libpmk), Cint, (Ptr{Cvoid}, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}), h[], C_NULL, C_NULL, inds),
          "pmk_model_patch_index")
    X_parts = [[X[:, inds[k] + 1] for k = off[r] + 1:off[r + 1]] for r = 1:P]
    η = MixtureGPType(X_parts, fetchhyperplanes(root))
    η.model = h[]; η.handle[] = h[]; η.N_global = N
    return η
end

"""fitmixtureGP!(η, y, θ, σ²) -> η on an η built by MixtureGPType(root, X, ε): y holds the targets of all N points; the
resident model gets them through its index list (pmk_model_set_targets_global) and is refitted.  No model is created."""
function fitmixtureGP!(η::MixtureGPType{Float64}, y::Vector{Float64}, θ, σ²)
    η.N_global > 0 || throw(ArgumentError("this η was built from lists of patches: pass y_parts, one vector per patch"))
    length(y) == η.N_global || throw(ArgumentError("one target per point: got $(length(y)) for $(η.N_global) points"))
    perpatchok(θ) || throw(ArgumentError("closure-carrying kernels are not available on an η built from a tree and global points"))
    P = length(η.X_parts); info = Vector{Int32}(undef, P)
    check(ccall((:pmk_model_set_targets_global, libpmk), Cint, (Ptr{Cvoid}, Ptr{Float64}), η.model, y), "pmk_model_set_targets_global")
    check(ccall((:pmk_model_fit, libpmk), Cint, (Ptr{Cvoid}, Ref{KernelDesc}, Float64), η.model, Ref(desc(θ)), σ²), "pmk_model_fit")
    check(ccall((:pmk_model_info, libpmk), Cint, (Ptr{Cvoid}, Ptr{Int32}), η.model, info), "pmk_model_info")
    empty!(η.U_set.cache); empty!(η.L_set.cache)
    bad = findfirst(!=(0), info)
    bad === nothing || throw(PosDefException(Int(info[bad])))       # cholesky(U) of mixtureGP.jl:109
    cs = [Vector{Float64}(undef, length(η.X_parts[r])) for r = 1:P]
    GC.@preserve cs check(ccall((:pmk_model_get_weights, libpmk), Cint, (Ptr{Cvoid}, Ptr{Ptr{Float64}}), η.model,
                                [pointer(c) for c in cs]), "pmk_model_get_weights")
    for r = 1:P
        η.c_set[r] = cs[r]
        η.σ²_set[r] = σ²
    end
    return η
end

function model_get(model::Ptr{Cvoid}, r::Int, what::Int, n::Int)
    out = what == 0 ? Vector{Float64}(undef, n) : Matrix{Float64}(undef, n, n)
    check(ccall((:pmk_model_get, libpmk), Cint, (Ptr{Cvoid}, Int64, Cint, Ptr{Float64}, Int64), model, r - 1, what, out, n),
          "pmk_model_get")
    return out
end

"""fitmixtureGP!(η, y_parts, θ, σ²) -> η (mixtureGP.jl:70-118).  c_set comes back to the host; U_set / L_set are read from
the device patch by patch when they are first indexed (LazyFactors); store_factors = true pulls all of them at once."""
function fitmixtureGP!(η::MixtureGPType{T}, y_parts::Vector{Vector{T}}, θ, σ²; store_factors::Bool = false) where T
    P = length(η.X_parts)
    # positions, or positions + warp values for a warp-feature kernel (the tree is built on the positions alone)
    Xm = [kpack(θ, X) for X in η.X_parts]; ys = [Vector{Float64}(y) for y in y_parts]
    n = Int64[size(x, 2) for x in Xm]; D = size(Xm[1], 1)
    for r = 1:P
        @assert length(ys[r]) == n[r]                      # mixtureGP.jl:298
    end
    if η.model != C_NULL
        ccall((:pmk_model_destroy, libpmk), Cvoid, (Ptr{Cvoid},), η.model)
        η.model = C_NULL; η.handle[] = C_NULL; η.N_global = 0
    end
    h = Ref{Ptr{Cvoid}}(C_NULL); info = Vector{Int32}(undef, P); d = Ref(desc(θ))
    gs = [diagaddend(θ, X) for X in η.X_parts]          # the DPP kernels' own diagonal term, else nothing
    if gs[1] === nothing
        GC.@preserve Xm ys begin
            rc = ccall((:pmk_fit_batched, libpmk), Cint,
                (Ptr{Cvoid}, Ref{KernelDesc}, Float64, Cint, Int64, Ptr{Int64}, Ptr{Ptr{Float64}}, Ptr{Ptr{Float64}},
                 Ref{Ptr{Cvoid}}, Ptr{Ptr{Float64}}, Ptr{Int32}),
                context(), d, σ², D, P, n, [pointer(x) for x in Xm], [pointer(y) for y in ys], h, C_NULL, info)
        end
        check(rc, "fitmixtureGP!")
    else
        GC.@preserve Xm ys gs begin
            check(ccall((:pmk_model_create, libpmk), Cint,
                (Ptr{Cvoid}, Cint, Int64, Ptr{Int64}, Ptr{Ptr{Float64}}, Ptr{Ptr{Float64}}, Ref{Ptr{Cvoid}}),
                context(), D, P, n, [pointer(x) for x in Xm], [pointer(y) for y in ys], h), "pmk_model_create")
            check(ccall((:pmk_model_set_diag, libpmk), Cint, (Ptr{Cvoid}, Ptr{Ptr{Float64}}), h[], [pointer(g) for g in gs]),
                  "pmk_model_set_diag")
            check(ccall((:pmk_model_fit, libpmk), Cint, (Ptr{Cvoid}, Ref{KernelDesc}, Float64), h[], d, σ²), "pmk_model_fit")
            check(ccall((:pmk_model_info, libpmk), Cint, (Ptr{Cvoid}, Ptr{Int32}), h[], info), "pmk_model_info")
        end
    end
    η.model = h[]
    η.handle[] = h[]
    empty!(η.U_set.cache); empty!(η.L_set.cache)
    η.U_set.n = Int.(n); η.L_set.n = Int.(n)
    bad = findfirst(!=(0), info)
    bad === nothing || throw(PosDefException(Int(info[bad])))       # cholesky(U) of mixtureGP.jl:109
    cs = [Vector{Float64}(undef, Int(n[r])) for r = 1:P]          # every c_r in one device-to-host transfer
    GC.@preserve cs check(ccall((:pmk_model_get_weights, libpmk), Cint, (Ptr{Cvoid}, Ptr{Ptr{Float64}}), η.model,
                                [pointer(c) for c in cs]), "pmk_model_get_weights")
    for r = 1:P
        η.c_set[r] = cs[r]
        η.σ²_set[r] = σ²
        if store_factors
            η.L_set[r]; η.U_set[r]                                  # pulled and cached
        end
    end
    return η
end

"""capacitymixtureGP(η) -> the points every patch can still take in place: ld_r - n_r, ld_r = 128 ceil(n_r / 128) until
reservemixtureGP! gives more."""
function capacitymixtureGP(η::MixtureGPType)
    η.model == C_NULL && throw(PMKError("fitmixtureGP! must run before capacitymixtureGP"))
    free = Vector{Int64}(undef, length(η.X_parts))
    check(ccall((:pmk_model_capacity, libpmk), Cint, (Ptr{Cvoid}, Ptr{Int64}), η.model, free), "pmk_model_capacity")
    return free
end

"""reservemixtureGP!(η, rows) -> η: afterwards every patch of the fitted η can take rows[r] more points (an Int: the same for
every patch) through appendmixtureGP!, across 128-row block boundaries, at most 128 per patch and call
(pmk_model_reserve).  Patches that lack the room get a larger stride: the model moves into a new layout and the old one
is freed; none is shrunk.  The fit is kept bit for bit.  Checked statically only, like the rest of this module."""
function reservemixtureGP!(η::MixtureGPType, rows::Union{Int,Vector{Int}})
    η.model == C_NULL && throw(PMKError("fitmixtureGP! must run before reservemixtureGP!"))
    P = length(η.X_parts)
    want = rows isa Int ? fill(Int64(rows), P) : Vector{Int64}(rows)
    length(want) == P || throw(ArgumentError("one number of rows per patch"))
    all(>=(0), want) || throw(ArgumentError("a negative number of rows"))
    check(ccall((:pmk_model_reserve, libpmk), Cint, (Ptr{Cvoid}, Ptr{Int64}), η.model, want), "pmk_model_reserve")
    η.R_multi = 0
    return η
end

"""appendmixtureGP!(η, X_new_parts, y_new_parts; global_index_parts) -> η: the new points X_new_parts[r] (empty entries
allowed) with targets y_new_parts[r] become the last rows of patch r of the fitted η, in place: the resident Cholesky
factor is bordered, not refitted (pmk_model_append).  On an η built by MixtureGPType(root, X, ε) the global index of every
new row is required (global_index_parts[r], 0-based, at least the old N and strictly ascending within a patch: the rows
follow the order given, and an order that does not ascend is refused; a point of several patches is a row in each).  c_set, L_set and U_set
follow; a failed new pivot throws PosDefException and leaves that patch failed until the next fit.  Kernels that carry a
closure are not served: their points carry more than the positions."""
function appendmixtureGP!(η::MixtureGPType{T}, X_new_parts::Vector{Vector{Vector{T}}}, y_new_parts::Vector{Vector{T}};
                          global_index_parts::Union{Nothing,Vector{Vector{Int}}} = nothing) where T
    η.model == C_NULL && throw(PMKError("fitmixtureGP! must run before appendmixtureGP!"))
    P = length(η.X_parts)
    length(X_new_parts) == P && length(y_new_parts) == P || throw(ArgumentError("one list of new points and targets per patch"))
    (η.N_global > 0) == (global_index_parts !== nothing) ||
        throw(ArgumentError("global_index_parts is required on an η built from a tree, and only there"))
    free = capacitymixtureGP(η)
    D = length(η.X_parts[1][1])
    x = Float64[]; y = Float64[]; patch = Int32[]; g = Int64[]
    for r = 1:P
        m = length(X_new_parts[r])
        length(y_new_parts[r]) == m || throw(ArgumentError("patch $r: $(length(y_new_parts[r])) targets for $m new points"))
        m <= free[r] || throw(ArgumentError("patch $r has $(free[r]) free rows, $m rows asked for"))
        for a = 1:m
            length(X_new_parts[r][a]) == D || throw(ArgumentError("patch $r: a new point of dimension $(length(X_new_parts[r][a])), not $D"))
            append!(x, X_new_parts[r][a]); push!(y, y_new_parts[r][a]); push!(patch, r - 1)
            global_index_parts === nothing || push!(g, global_index_parts[r][a])
        end
    end
    isempty(y) && return η
    all(isfinite, x) && all(isfinite, y) || throw(ArgumentError("non-finite coordinate or target"))
    check(ccall((:pmk_model_append, libpmk), Cint,
        (Ptr{Cvoid}, Int64, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Int32}, Ptr{Int64}),
        η.model, length(y), x, y, C_NULL, patch, global_index_parts === nothing ? C_NULL : g), "pmk_model_append")
    for r = 1:P
        append!(η.X_parts[r], X_new_parts[r])
    end
    η.N_global > 0 && (η.N_global = max(η.N_global, maximum(g) + 1))
    η.R_multi = 0
    n = Int[length(X) for X in η.X_parts]
    empty!(η.U_set.cache); empty!(η.L_set.cache)
    η.U_set.n = n; η.L_set.n = n
    info = Vector{Int32}(undef, P)
    check(ccall((:pmk_model_info, libpmk), Cint, (Ptr{Cvoid}, Ptr{Int32}), η.model, info), "pmk_model_info")
    cs = [Vector{Float64}(undef, n[r]) for r = 1:P]
    GC.@preserve cs check(ccall((:pmk_model_get_weights, libpmk), Cint, (Ptr{Cvoid}, Ptr{Ptr{Float64}}), η.model,
                                [pointer(c) for c in cs]), "pmk_model_get_weights")
    for r = 1:P
        η.c_set[r] = cs[r]
    end
    bad = findfirst(!=(0), info)
    bad === nothing || throw(PosDefException(Int(info[bad])))
    return η
end

"""removablemixtureGP(η) -> the rows every patch can still lose in place: n_r - 128 (ceil(n_r / 128) - 1) - 1 (a patch stays
in its last block row of 128)."""
function removablemixtureGP(η::MixtureGPType)
    η.model == C_NULL && throw(PMKError("fitmixtureGP! must run before removablemixtureGP"))
    rows = Vector{Int64}(undef, length(η.X_parts))
    check(ccall((:pmk_model_removable, libpmk), Cint, (Ptr{Cvoid}, Ptr{Int64}), η.model, rows), "pmk_model_removable")
    return rows
end

"""removemixtureGP!(η, rows_parts) -> η: the rows rows_parts[r] (ONE-based indices into η.X_parts[r] as it stands before
the call, empty entries allowed, any order) leave patch r of the fitted η, in place: the rows are deleted from the
resident Cholesky factor, which is not refitted (pmk_model_remove); at most 32 rows of one patch a call.  On an η built
by MixtureGPType(root, X, ε) a global point of several patches is a row in each, and the library's index list follows;
N does not change.  c_set, L_set, U_set and X_parts follow; a failed new diagonal throws PosDefException and leaves that
patch failed until the next fit.  Checked statically only, like the rest of this module."""
function removemixtureGP!(η::MixtureGPType{T}, rows_parts::Vector{Vector{Int}}) where T
    η.model == C_NULL && throw(PMKError("fitmixtureGP! must run before removemixtureGP!"))
    P = length(η.X_parts)
    length(rows_parts) == P || throw(ArgumentError("one list of rows per patch"))
    can = removablemixtureGP(η)
    patch = Int32[]; row = Int64[]
    for r = 1:P
        rows = sort(rows_parts[r])
        allunique(rows) || throw(ArgumentError("patch $r: a row is given twice"))
        isempty(rows) || (1 <= rows[1] && rows[end] <= length(η.X_parts[r])) ||
            throw(ArgumentError("patch $r: a row outside 1 .. $(length(η.X_parts[r]))"))
        length(rows) <= can[r] || throw(ArgumentError("patch $r has $(can[r]) removable rows, $(length(rows)) rows asked for"))
        for i in rows
            push!(patch, r - 1); push!(row, i - 1)
        end
    end
    isempty(row) && return η
    check(ccall((:pmk_model_remove, libpmk), Cint, (Ptr{Cvoid}, Int64, Ptr{Int32}, Ptr{Int64}),
        η.model, length(row), patch, row), "pmk_model_remove")
    for r = 1:P
        deleteat!(η.X_parts[r], sort(rows_parts[r]))
    end
    η.R_multi = 0
    n = Int[length(X) for X in η.X_parts]
    empty!(η.U_set.cache); empty!(η.L_set.cache)
    η.U_set.n = n; η.L_set.n = n
    info = Vector{Int32}(undef, P)
    check(ccall((:pmk_model_info, libpmk), Cint, (Ptr{Cvoid}, Ptr{Int32}), η.model, info), "pmk_model_info")
    cs = [Vector{Float64}(undef, n[r]) for r = 1:P]
    GC.@preserve cs check(ccall((:pmk_model_get_weights, libpmk), Cint, (Ptr{Cvoid}, Ptr{Ptr{Float64}}), η.model,
                                [pointer(c) for c in cs]), "pmk_model_get_weights")
    for r = 1:P
        η.c_set[r] = cs[r]
    end
    bad = findfirst(!=(0), info)
    bad === nothing || throw(PosDefException(Int(info[bad])))
    return η
end

"""querymixtureGP!(Yq, Vq, Xq, η, root, levels, radius, δ, θ, σ², weight_θ, debug_vars; debug_flag)
(mixtureGP.jl:159-294)"""
function querymixtureGP!(Yq::Vector{T}, Vq::Vector{T}, Xq::Vector{Vector{T}}, η::MixtureGPType{T}, root, levels,
                         radius::T, δ::T, θ, σ², weight_θ, debug_vars::MixtureGPDebugType{T};
                         debug_flag = false)::Nothing where T
    η.model == C_NULL && throw(PMKError("fitmixtureGP! must run before querymixtureGP!"))
    Nq = length(Xq); Xm = kpack(θ, Xq)                         # positions (+ warp values): the tree uses the positions
    resize!(Yq, Nq); resize!(Vq, Nq)                          # mixtureGP.jl:179-180
    check(ccall((:pmk_model_set_bsp, libpmk), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Int64), η.model, native(root), 0), "pmk_model_set_bsp")
    q = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:pmk_query_create, libpmk), Cint, (Ptr{Cvoid}, Int64, Ptr{Float64}, Ref{Ptr{Cvoid}}), η.model, Nq, Xm, q), "pmk_query_create")
    try
        gq = diagaddend(θ, Xq)
        gq === nothing || check(ccall((:pmk_query_set_diag, libpmk), Cint, (Ptr{Cvoid}, Ptr{Float64}), q[], gq), "pmk_query_set_diag")
        check(ccall((:pmk_query_plan, libpmk), Cint, (Ptr{Cvoid}, Float64, Float64), q[], radius, δ), "pmk_query_plan")
        check(ccall((:pmk_query_items, libpmk), Cint, (Ptr{Cvoid}, Ref{KernelDesc}), q[], Ref(desc(θ))), "pmk_query_items")
        check(ccall((:pmk_query_mix, libpmk), Cint, (Ptr{Cvoid}, Ref{KernelDesc}, Int64, Int64), q[], Ref(desc(weight_θ)), 0, Nq), "pmk_query_mix")
        check(ccall((:pmk_query_fetch, libpmk), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}), q[], Yq, Vq), "pmk_query_fetch")
        if debug_flag
            tot = Ref{Int64}(0)
            check(ccall((:pmk_query_counts, libpmk), Cint, (Ptr{Cvoid}, Ref{Int64}, Ptr{Int64}, Ptr{Int64}), q[], tot, C_NULL, C_NULL), "pmk_query_counts")
            home = Vector{Int64}(undef, Nq); off = Vector{Int64}(undef, Nq + 1); reg = Vector{Int64}(undef, max(tot[], 1))
            t = Vector{Float64}(undef, max(tot[], 1)); w = similar(t); u = similar(t); v = similar(t)
            check(ccall((:pmk_query_debug, libpmk), Cint,
                (Ptr{Cvoid}, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                q[], home, off, reg, t, w, u, v), "pmk_query_debug")
            # the reference resize!s every field to Nq and assigns (mixtureGP.jl:185-195): a reused struct does not grow
            resize!(debug_vars.w_tilde_set, Nq); resize!(debug_vars.u_set, Nq); resize!(debug_vars.v_set, Nq)
            resize!(debug_vars.region_inds_set, Nq); resize!(debug_vars.p_region_ind_set, Nq)
            resize!(debug_vars.hps_keep_flags_set, Nq); resize!(debug_vars.zs_set, Nq); resize!(debug_vars.ts_set, Nq)
            for j = 1:Nq
                s = off[j]+1:off[j+1]
                debug_vars.w_tilde_set[j] = w[s]; debug_vars.u_set[j] = u[s]; debug_vars.v_set[j] = v[s]
                debug_vars.region_inds_set[j] = Vector{Int}(reg[s[1:end-1]] .+ 1)
                debug_vars.p_region_ind_set[j] = Int(home[j]) + 1
                _, ts, zs, keep = findneighbourpartitions(Xq[j], radius, root, levels, η.hps, Int(home[j]) + 1; δ = δ)
                debug_vars.hps_keep_flags_set[j] = keep; debug_vars.zs_set[j] = zs; debug_vars.ts_set[j] = ts
            end
        end
    finally
        ccall((:pmk_query_destroy, libpmk), Cvoid, (Ptr{Cvoid},), q[])
    end
    return nothing
end

# ------------------------------------------------------------------------------------------ multi-output targets
"""fitmixtureGPmulti!(η, Y_parts, θ, σ²) -> C_set: fitmixtureGP! (mixtureGP.jl:70-118) with R target columns per patch
(Y_parts[r] is n_r x R, 1 <= R <= 16) that share one factor.  The fit runs once on column 1 (η.c_set, η.L_set as
fitmixtureGP! leaves them); every column is then solved from the resident factor (c = U \\ y of mixtureGP.jl:106 for R
right-hand sides, pmk_model_solve_multi).  Returns the n_r x R weights of every patch."""
function fitmixtureGPmulti!(η::MixtureGPType{T}, Y_parts::Vector{Matrix{T}}, θ, σ²::T) where T
    P = length(η.X_parts)
    length(Y_parts) == P || throw(ArgumentError("one target matrix per patch"))
    R = size(Y_parts[1], 2)
    1 <= R <= 16 || throw(ArgumentError("R = $R target columns, outside 1..16"))
    for r = 1:P
        size(Y_parts[r]) == (length(η.X_parts[r]), R) || throw(ArgumentError("patch $r: targets must be n x $R"))
    end
    fitmixtureGP!(η, [Y[:, 1] for Y in Y_parts], θ, σ²)
    Ys = [Matrix{Float64}(Y) for Y in Y_parts]
    ldy = Int64[size(Y, 1) for Y in Ys]
    GC.@preserve Ys begin
        check(ccall((:pmk_model_set_targets_multi, libpmk), Cint, (Ptr{Cvoid}, Cint, Ptr{Ptr{Float64}}, Ptr{Int64}),
                    η.model, R, [pointer(Y) for Y in Ys], ldy), "pmk_model_set_targets_multi")
    end
    η.R_multi = R
    check(ccall((:pmk_model_solve_multi, libpmk), Cint, (Ptr{Cvoid},), η.model), "pmk_model_solve_multi")
    Cs = [Matrix{Float64}(undef, size(Y, 1), R) for Y in Ys]
    GC.@preserve Cs check(ccall((:pmk_model_get_weights_multi, libpmk), Cint, (Ptr{Cvoid}, Ptr{Ptr{Float64}}, Ptr{Int64}),
                                η.model, [pointer(c) for c in Cs], ldy), "pmk_model_get_weights_multi")
    return Cs
end

"""querymixtureGPmulti!(Yq, Vq, Xq, η, root, levels, radius, δ, θ, σ², weight_θ): querymixtureGP! (mixtureGP.jl:159-294)
for the R columns of fitmixtureGPmulti!.  Yq is Nq x R (R of the fit); Vq is resized to Nq, and Vq === nothing skips the
variance (no triangular solve: the means need only kq . C, queryinner! of mixtureGP.jl:296-316)."""
function querymixtureGPmulti!(Yq::Matrix{T}, Vq::Union{Vector{T},Nothing}, Xq::Vector{Vector{T}}, η::MixtureGPType{T}, root,
                              levels, radius::T, δ::T, θ, σ², weight_θ)::Nothing where T
    η.model == C_NULL && throw(PMKError("fitmixtureGPmulti! must run before querymixtureGPmulti!"))
    Nq = length(Xq); Xm = kpack(θ, Xq)
    size(Yq, 1) == Nq && 1 <= size(Yq, 2) <= 16 || throw(ArgumentError("Yq must be length(Xq) x R"))
    Ym = Matrix{Float64}(undef, Nq, 16)          # room for any R <= PMK_MAX_OUTPUTS: the library writes the fit's R columns
    Vq === nothing || resize!(Vq, Nq)
    check(ccall((:pmk_model_set_bsp, libpmk), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Int64), η.model, native(root), 0), "pmk_model_set_bsp")
    q = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:pmk_query_create, libpmk), Cint, (Ptr{Cvoid}, Int64, Ptr{Float64}, Ref{Ptr{Cvoid}}), η.model, Nq, Xm, q), "pmk_query_create")
    try
        gq = diagaddend(θ, Xq)
        gq === nothing || check(ccall((:pmk_query_set_diag, libpmk), Cint, (Ptr{Cvoid}, Ptr{Float64}), q[], gq), "pmk_query_set_diag")
        check(ccall((:pmk_query_plan, libpmk), Cint, (Ptr{Cvoid}, Float64, Float64), q[], radius, δ), "pmk_query_plan")
        check(ccall((:pmk_query_items_multi, libpmk), Cint, (Ptr{Cvoid}, Ref{KernelDesc}, Cint), q[], Ref(desc(θ)),
                    Vq === nothing ? 0 : 1), "pmk_query_items_multi")
        check(ccall((:pmk_query_mix_multi, libpmk), Cint, (Ptr{Cvoid}, Ref{KernelDesc}, Int64, Int64), q[], Ref(desc(weight_θ)), 0, Nq),
              "pmk_query_mix_multi")
        check(ccall((:pmk_query_fetch_multi, libpmk), Cint, (Ptr{Cvoid}, Ptr{Float64}, Int64, Ptr{Float64}), q[], Ym, max(Nq, 1),
                    Vq === nothing ? Ptr{Float64}(C_NULL) : pointer(Vq)), "pmk_query_fetch_multi")
    finally
        ccall((:pmk_query_destroy, libpmk), Cvoid, (Ptr{Cvoid},), q[])
    end
    Yq .= view(Ym, :, 1:size(Yq, 2))
    return nothing
end

# ------------------------------------------------------------------------------------------ model selection
# Is this (θ, σ²) any good on this patch?  Two scores from the factor that fitmixtureGP! left on the device (Rasmussen &
# Williams, eq. 5.8 and 5.10-5.12).  Both are PER PATCH: overlapping ε-sets put a training point into several patches, and
# it has one score in each.  A patch whose factorisation failed returns NaN.
"""logevidencemixtureGP(η) -> Vector of the P log marginal likelihoods -½ yᵀc - ½ log det(K + σ²I) - (n/2) log 2π"""
function logevidencemixtureGP(η::MixtureGPType{T}) where T
    η.model == C_NULL && throw(PMKError("fitmixtureGP! must run before logevidencemixtureGP"))
    P = length(η.X_parts)
    logdet = Vector{Float64}(undef, P); quad = Vector{Float64}(undef, P)
    check(ccall((:pmk_model_evidence, libpmk), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}), η.model, logdet, quad),
          "pmk_model_evidence")
    return [-0.5 * quad[r] - 0.5 * logdet[r] - 0.5 * length(η.X_parts[r]) * log(2π) for r = 1:P]
end

"""logevidencemixtureGPmulti(η, R) -> P x R matrix, for the R columns of fitmixtureGPmulti! (one log det per patch
serves every column)"""
function logevidencemixtureGPmulti(η::MixtureGPType{T}, R::Integer) where T
    η.model == C_NULL && throw(PMKError("fitmixtureGPmulti! must run before logevidencemixtureGPmulti"))
    1 <= R <= 16 || throw(ArgumentError("R = $R target columns, outside 1..16"))
    P = length(η.X_parts)
    logdet = Vector{Float64}(undef, P); quad = Matrix{Float64}(undef, P, 16)    # room for any R <= PMK_MAX_OUTPUTS
    check(ccall((:pmk_model_evidence_multi, libpmk), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}), η.model, logdet, quad),
          "pmk_model_evidence_multi")
    return [-0.5 * quad[r, j] - 0.5 * logdet[r] - 0.5 * length(η.X_parts[r]) * log(2π) for r = 1:P, j = 1:R]
end

"""loomixtureGP(η) -> (res_set, var_set): leave-one-out residuals and variances of every training point of every patch,
from one pass over the resident factor (no refit).  res_set[r][i] = yᵢ - μ₋ᵢ (so μ₋ᵢ = yᵢ - res_set[r][i]);
var_set[r][i] is the predictive variance of yᵢ from the other n_r - 1 points of patch r, noise included."""
function loomixtureGP(η::MixtureGPType{T}) where T
    η.model == C_NULL && throw(PMKError("fitmixtureGP! must run before loomixtureGP"))
    check(ccall((:pmk_model_loo, libpmk), Cint, (Ptr{Cvoid},), η.model), "pmk_model_loo")
    res = [Vector{Float64}(undef, length(X)) for X in η.X_parts]
    var = [Vector{Float64}(undef, length(X)) for X in η.X_parts]
    GC.@preserve res var check(ccall((:pmk_model_get_loo, libpmk), Cint, (Ptr{Cvoid}, Ptr{Ptr{Float64}}, Ptr{Ptr{Float64}}),
                                     η.model, [pointer(a) for a in res], [pointer(a) for a in var]), "pmk_model_get_loo")
    return res, var
end

"""loomixtureGPmulti(η, R) -> (RES_set, var_set) for the R columns of fitmixtureGPmulti!: RES_set[r] is n_r x R, the
variances are shared by the columns"""
function loomixtureGPmulti(η::MixtureGPType{T}, R::Integer) where T
    η.model == C_NULL && throw(PMKError("fitmixtureGPmulti! must run before loomixtureGPmulti"))
    1 <= R <= 16 || throw(ArgumentError("R = $R target columns, outside 1..16"))
    check(ccall((:pmk_model_loo, libpmk), Cint, (Ptr{Cvoid},), η.model), "pmk_model_loo")
    RES = [Matrix{Float64}(undef, length(X), 16) for X in η.X_parts]            # room for any R <= PMK_MAX_OUTPUTS
    var = [Vector{Float64}(undef, length(X)) for X in η.X_parts]
    ldres = Int64[size(A, 1) for A in RES]
    GC.@preserve RES var check(ccall((:pmk_model_get_loo_multi, libpmk), Cint,
                                     (Ptr{Cvoid}, Ptr{Ptr{Float64}}, Ptr{Int64}, Ptr{Ptr{Float64}}),
                                     η.model, [pointer(A) for A in RES], ldres, [pointer(a) for a in var]), "pmk_model_get_loo_multi")
    return [A[:, 1:R] for A in RES], var
end

"""loomixtureGP_blend(η, root, radius, δ, weight_θ, X; noisy = false, counts = false) -> (μ, v): the leave-one-out of the
BLENDED predictor at every training point, without refitting: what querymixtureGP! would predict at column j of X had η
been fitted without point j, the tree held fixed.  η: built by MixtureGPType(root, X, ε) and fitted; X: the same D x N
matrix.  An item whose patch holds the point comes from the resident leave-one-out values (pmk_model_loo, run here), any
other item from the strips (pmk_query_items_loo).  noisy: variances of the observation (each patch's σ² included) rather
than of the latent field.  counts = true runs the staged calls and returns (μ, v, n_member, n_strip)."""
function loomixtureGP_blend(η::MixtureGPType{Float64}, root, radius::Float64, δ::Float64, weight_θ, X::Matrix{Float64};
                            noisy::Bool = false, counts::Bool = false)
    η.model == C_NULL && throw(PMKError("fitmixtureGP! must run before loomixtureGP_blend"))
    η.N_global > 0 || throw(ArgumentError("this η was built from lists of patches: build it with MixtureGPType(root, X, ε)"))
    N = size(X, 2)
    N == η.N_global || throw(ArgumentError("X has $N points, the model $(η.N_global)"))
    μ = Vector{Float64}(undef, N); v = Vector{Float64}(undef, N)
    check(ccall((:pmk_model_loo, libpmk), Cint, (Ptr{Cvoid},), η.model), "pmk_model_loo")
    if !counts
        check(ccall((:pmk_predict_mixture_loo, libpmk), Cint,
                    (Ptr{Cvoid}, Ref{KernelDesc}, Ptr{Float64}, Float64, Float64, Cint, Ptr{Float64}, Ptr{Float64}),
                    η.model, Ref(desc(weight_θ)), X, radius, δ, noisy ? 1 : 0, μ, v), "pmk_predict_mixture_loo")
        return μ, v
    end
    q = Ref{Ptr{Cvoid}}(C_NULL); nm = Ref{Int64}(0); ns = Ref{Int64}(0)
    check(ccall((:pmk_query_create, libpmk), Cint, (Ptr{Cvoid}, Int64, Ptr{Float64}, Ref{Ptr{Cvoid}}), η.model, N, X, q), "pmk_query_create")
    try
        check(ccall((:pmk_query_plan, libpmk), Cint, (Ptr{Cvoid}, Float64, Float64), q[], radius, δ), "pmk_query_plan")
        check(ccall((:pmk_query_items_loo, libpmk), Cint, (Ptr{Cvoid}, Cint, Ref{Int64}, Ref{Int64}), q[], noisy ? 1 : 0, nm, ns),
              "pmk_query_items_loo")
        check(ccall((:pmk_query_mix, libpmk), Cint, (Ptr{Cvoid}, Ref{KernelDesc}, Int64, Int64), q[], Ref(desc(weight_θ)), 0, N), "pmk_query_mix")
        check(ccall((:pmk_query_fetch, libpmk), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}), q[], μ, v), "pmk_query_fetch")
    finally
        ccall((:pmk_query_destroy, libpmk), Cvoid, (Ptr{Cvoid},), q[])
    end
    return μ, v, nm[], ns[]
end

"""loomixtureGP_blend_multi(η, root, radius, δ, weight_θ, X; noisy = false, variance = true, items = false) -> (M, v): the
leave-one-out of the BLENDED predictor for the R target columns of fitmixtureGPmulti!, with the trend of
settrendmixtureGP! if one is set: M is N x R, v the N variances (nothing with variance = false: no strip kernel runs).
η: built by MixtureGPType(root, X, ε), fitted, and solved (fitmixtureGPmulti! / settrendmixtureGP!); X: the same D x N
matrix.  An item whose patch holds the point comes from the resident values (pmk_model_loo, run here), any other item is
that of pmk_query_items_multi_fitted.  items = true runs the staged calls and returns
(M, v, n_member, n_other, U, vi): U is R x total, the per-item means in the item order of the plan, vi their variances."""
function loomixtureGP_blend_multi(η::MixtureGPType{Float64}, root, radius::Float64, δ::Float64, weight_θ, X::Matrix{Float64};
                                  noisy::Bool = false, variance::Bool = true, items::Bool = false)
    η.model == C_NULL && throw(PMKError("fitmixtureGPmulti! must run before loomixtureGP_blend_multi"))
    η.N_global > 0 || throw(ArgumentError("this η was built from lists of patches: build it with MixtureGPType(root, X, ε)"))
    R = η.R_multi
    R >= 1 || throw(PMKError("fitmixtureGPmulti! must run before loomixtureGP_blend_multi"))
    N = size(X, 2)
    N == η.N_global || throw(ArgumentError("X has $N points, the model $(η.N_global)"))
    M = Matrix{Float64}(undef, N, R); v = Vector{Float64}(undef, variance ? N : 0)
    vp = variance ? pointer(v) : Ptr{Float64}(C_NULL)
    check(ccall((:pmk_model_loo, libpmk), Cint, (Ptr{Cvoid},), η.model), "pmk_model_loo")
    if !items
        GC.@preserve v check(ccall((:pmk_predict_mixture_loo_multi, libpmk), Cint,
                    (Ptr{Cvoid}, Ref{KernelDesc}, Ptr{Float64}, Float64, Float64, Cint, Ptr{Float64}, Int64, Ptr{Float64}),
                    η.model, Ref(desc(weight_θ)), X, radius, δ, noisy ? 1 : 0, M, N, vp), "pmk_predict_mixture_loo_multi")
        return M, (variance ? v : nothing)
    end
    q = Ref{Ptr{Cvoid}}(C_NULL); nm = Ref{Int64}(0); no = Ref{Int64}(0); total = Ref{Int64}(0)
    check(ccall((:pmk_query_create, libpmk), Cint, (Ptr{Cvoid}, Int64, Ptr{Float64}, Ref{Ptr{Cvoid}}), η.model, N, X, q), "pmk_query_create")
    try
        check(ccall((:pmk_query_plan, libpmk), Cint, (Ptr{Cvoid}, Float64, Float64), q[], radius, δ), "pmk_query_plan")
        check(ccall((:pmk_query_counts, libpmk), Cint, (Ptr{Cvoid}, Ref{Int64}, Ptr{Int64}, Ptr{Int64}), q[], total,
                    Ptr{Int64}(C_NULL), Ptr{Int64}(C_NULL)), "pmk_query_counts")
        check(ccall((:pmk_query_items_loo_multi, libpmk), Cint, (Ptr{Cvoid}, Cint, Cint, Ref{Int64}, Ref{Int64}), q[],
                    noisy ? 1 : 0, variance ? 1 : 0, nm, no), "pmk_query_items_loo_multi")
        check(ccall((:pmk_query_mix_multi, libpmk), Cint, (Ptr{Cvoid}, Ref{KernelDesc}, Int64, Int64), q[], Ref(desc(weight_θ)), 0, N),
              "pmk_query_mix_multi")
        GC.@preserve v check(ccall((:pmk_query_fetch_multi, libpmk), Cint, (Ptr{Cvoid}, Ptr{Float64}, Int64, Ptr{Float64}), q[], M, N, vp),
                             "pmk_query_fetch_multi")
        U = Matrix{Float64}(undef, R, total[]); vi = Vector{Float64}(undef, variance ? total[] : 0)
        vip = variance ? pointer(vi) : Ptr{Float64}(C_NULL)
        GC.@preserve vi check(ccall((:pmk_query_get_items_multi, libpmk), Cint, (Ptr{Cvoid}, Ptr{Float64}, Int64, Ptr{Float64}), q[], U, R,
                                    vip), "pmk_query_get_items_multi")
        return M, (variance ? v : nothing), nm[], no[], U, (variance ? vi : nothing)
    finally
        ccall((:pmk_query_destroy, libpmk), Cvoid, (Ptr{Cvoid},), q[])
    end
end

"""selectblendGP_multi!(η, root, Y, candidates, X) -> (scores, best): score blending settings by the leave-one-out log
pseudo-likelihood of the blended predictor.  candidates: a vector of (radius, δ, weight_θ); Y: the N x R global targets the
model holds; scores[g, c] = Σⱼ [-½ log vⱼ - (Y[j, c] - M_g[j, c])² / (2 vⱼ) - ½ log 2π] with the noisy variances; best is
the first argmax of the row sums, a row with a NaN never wins.  The fit is not touched."""
function selectblendGP_multi!(η::MixtureGPType{Float64}, root, Y::Matrix{Float64}, candidates::Vector, X::Matrix{Float64})
    isempty(candidates) && throw(ArgumentError("no candidates"))
    R = η.R_multi
    size(Y) == (size(X, 2), R) || throw(ArgumentError("Y must be N x R with the model's R = $R target columns"))
    scores = Matrix{Float64}(undef, length(candidates), R)
    for (g, (radius, δ, weight_θ)) in enumerate(candidates)
        M, v = loomixtureGP_blend_multi(η, root, Float64(radius), Float64(δ), weight_θ, X; noisy = true)
        for c = 1:R
            scores[g, c] = sum(-0.5 .* log.(v) .- (Y[:, c] .- M[:, c]) .^ 2 ./ (2.0 .* v) .- 0.5 * log(2π))
        end
    end
    rows = vec(sum(scores, dims = 2))
    valid = findall(!isnan, rows)
    isempty(valid) && throw(ArgumentError("every candidate scored NaN"))
    return scores, valid[argmax(rows[valid])]
end

# ------------------------------------------------------------------------------------------ kriging with a trend
# One generalised-least-squares drift per patch on the multi-output path (include/pmk.h): :none is simple kriging (the
# default), :constant ordinary kriging (h = [1]), :linear universal kriging with h(x) = [1, x₁ … x_D] in the raw, uncentred
# coordinates.  The single-output calls ignore it.
"""settrendmixtureGP!(η, R, trend) -> C_set: set the trend of the fitted η (:none, :constant or :linear) and solve the R
target columns of fitmixtureGPmulti! again from the resident factor; returns the n_r x R weights (the universal-kriging
weights with a trend).  querymixtureGPmulti!, logevidencemixtureGPmulti and loomixtureGPmulti then serve unchanged.
Throws if R + q > 16 or if a patch is flagged (trendinfomixtureGP)."""
function settrendmixtureGP!(η::MixtureGPType{T}, R::Integer, trend::Symbol) where T
    η.model == C_NULL && throw(PMKError("fitmixtureGPmulti! must run before settrendmixtureGP!"))
    trend in (:none, :constant, :linear) || throw(ArgumentError("trend must be :none, :constant or :linear"))
    R == η.R_multi || throw(ArgumentError("R = $R, but fitmixtureGPmulti! set $(η.R_multi) target columns"))
    degree = trend === :none ? -1 : trend === :constant ? 0 : 1
    check(ccall((:pmk_model_set_trend, libpmk), Cint, (Ptr{Cvoid}, Cint), η.model, degree), "pmk_model_set_trend")
    check(ccall((:pmk_model_solve_multi, libpmk), Cint, (Ptr{Cvoid},), η.model), "pmk_model_solve_multi")
    flags = trendinfomixtureGP(η)
    any(flags .!= 0) && throw(PMKError("the trend basis of patch $(findfirst(flags .!= 0)) is rank deficient"))
    Cs = [Matrix{Float64}(undef, length(X), R) for X in η.X_parts]
    ldc = Int64[size(c, 1) for c in Cs]
    GC.@preserve Cs check(ccall((:pmk_model_get_weights_multi, libpmk), Cint, (Ptr{Cvoid}, Ptr{Ptr{Float64}}, Ptr{Int64}),
                                η.model, [pointer(c) for c in Cs], ldc), "pmk_model_get_weights_multi")
    return Cs
end

"""trendmixtureGP(η, R) -> (β_set, G_set): β_set[r] is q x R (coefficients of [1, x₁ … x_D] for every target column of
patch r), G_set[r] = HᵀU⁻¹H (q x q; its conditioning is the caller's to judge, log det G enters a restricted likelihood).
q = 0 without a trend."""
function trendmixtureGP(η::MixtureGPType{T}, R::Integer) where T
    η.model == C_NULL && throw(PMKError("fitmixtureGPmulti! must run before trendmixtureGP"))
    R == η.R_multi || throw(ArgumentError("R = $R, but fitmixtureGPmulti! set $(η.R_multi) target columns"))
    P = length(η.X_parts)
    q = Ref{Cint}(0)
    check(ccall((:pmk_model_get_trend, libpmk), Cint, (Ptr{Cvoid}, Ref{Cint}, Ptr{Float64}, Ptr{Float64}), η.model, q,
                Ptr{Float64}(C_NULL), Ptr{Float64}(C_NULL)), "pmk_model_get_trend")
    nq = Int(q[])
    β = Array{Float64}(undef, nq, R, P); G = Array{Float64}(undef, nq, nq, P)
    nq > 0 && check(ccall((:pmk_model_get_trend, libpmk), Cint, (Ptr{Cvoid}, Ref{Cint}, Ptr{Float64}, Ptr{Float64}), η.model, q,
                          β, G), "pmk_model_get_trend")
    return [β[:, :, r] for r = 1:P], [G[:, :, r] for r = 1:P]
end

"""trendinfomixtureGP(η) -> Vector{Int32} of the P per-patch flags: 0 ok, a in 1..q: pivot a of the Cholesky of G failed,
n_r + 1: the patch has fewer points than basis functions"""
function trendinfomixtureGP(η::MixtureGPType{T}) where T
    η.model == C_NULL && throw(PMKError("fitmixtureGPmulti! must run before trendinfomixtureGP"))
    flags = Vector{Int32}(undef, length(η.X_parts))
    rc = ccall((:pmk_model_trend_info, libpmk), Cint, (Ptr{Cvoid}, Ptr{Int32}), η.model, flags)
    rc < 0 && check(rc, "pmk_model_trend_info")
    return flags
end

# ------------------------------------------------------------------------------------------ per-patch kernels and noise
# MixtureGPType carries one σ² per patch (σ²_set, mixtureGP.jl:44,114) and the reference fills it with one value.  Here
# every patch may have its own θ and σ², which is what the per-patch scores above are for.  weight_θ stays global.
# Closure-carrying kernels are refused: their warp features change the model's D, and a mix of them is not meaningful.
perpatchok(θ) = !(θ isa WarpedKernel)

"""fitmixtureGP!(η, y_parts, θs, σ²s) -> η: fitmixtureGP! (mixtureGP.jl:70-118) with θs[r], σ²s[r] for patch r
(pmk_model_fit_patches).  Fills η.σ²_set[r] with the patch's own value and η.θ_set."""
function fitmixtureGP!(η::MixtureGPType{T}, y_parts::Vector{Vector{T}}, θs::Vector, σ²s::Vector) where T
    P = length(η.X_parts)
    length(θs) == P || throw(ArgumentError("one kernel per patch: got $(length(θs)) for $P patches"))
    length(σ²s) == P || throw(ArgumentError("one noise variance per patch: got $(length(σ²s)) for $P patches"))
    all(perpatchok, θs) || throw(ArgumentError("closure-carrying kernels cannot be set per patch"))
    Xm = [array2matrix(X) for X in η.X_parts]; ys = [Vector{Float64}(y) for y in y_parts]
    n = Int64[size(x, 2) for x in Xm]; D = size(Xm[1], 1)
    if η.model != C_NULL
        ccall((:pmk_model_destroy, libpmk), Cvoid, (Ptr{Cvoid},), η.model)
        η.model = C_NULL; η.handle[] = C_NULL; η.N_global = 0
    end
    h = Ref{Ptr{Cvoid}}(C_NULL); info = Vector{Int32}(undef, P)
    ds = KernelDesc[desc(θ) for θ in θs]; s2 = Vector{Float64}(σ²s)
    GC.@preserve Xm ys begin
        check(ccall((:pmk_model_create, libpmk), Cint,
            (Ptr{Cvoid}, Cint, Int64, Ptr{Int64}, Ptr{Ptr{Float64}}, Ptr{Ptr{Float64}}, Ref{Ptr{Cvoid}}),
            context(), D, P, n, [pointer(x) for x in Xm], [pointer(y) for y in ys], h), "pmk_model_create")
    end
    η.model = h[]
    η.handle[] = h[]
    check(ccall((:pmk_model_fit_patches, libpmk), Cint, (Ptr{Cvoid}, Ptr{KernelDesc}, Ptr{Float64}), η.model, ds, s2),
          "pmk_model_fit_patches")
    check(ccall((:pmk_model_info, libpmk), Cint, (Ptr{Cvoid}, Ptr{Int32}), η.model, info), "pmk_model_info")
    empty!(η.U_set.cache); empty!(η.L_set.cache)
    η.U_set.n = Int.(n); η.L_set.n = Int.(n)
    bad = findfirst(!=(0), info)
    bad === nothing || throw(PosDefException(Int(info[bad])))       # cholesky(U) of mixtureGP.jl:109
    cs = [Vector{Float64}(undef, Int(n[r])) for r = 1:P]
    GC.@preserve cs check(ccall((:pmk_model_get_weights, libpmk), Cint, (Ptr{Cvoid}, Ptr{Ptr{Float64}}), η.model,
                                [pointer(c) for c in cs]), "pmk_model_get_weights")
    η.θ_set = Any[θ for θ in θs]
    for r = 1:P
        η.c_set[r] = cs[r]
        η.σ²_set[r] = σ²s[r]
    end
    return η
end

"""gethyper(η) -> (descs, σ²s): the hyperparameters the resident factor belongs to (pmk_model_get_hyper)"""
function gethyper(η::MixtureGPType{T}) where T
    η.model == C_NULL && throw(PMKError("fitmixtureGP! must run before gethyper"))
    P = length(η.X_parts)
    ds = Vector{KernelDesc}(undef, P); s2 = Vector{Float64}(undef, P)
    check(ccall((:pmk_model_get_hyper, libpmk), Cint, (Ptr{Cvoid}, Ptr{KernelDesc}, Ptr{Float64}), η.model, ds, s2),
          "pmk_model_get_hyper")
    return ds, s2
end

"""querymixtureGP!(Yq, Vq, Xq, η, root, levels, radius, δ, weight_θ): querymixtureGP! (mixtureGP.jl:159-294) with the
model's own kernels, region r with the θ it was fitted with (pmk_predict_mixture_fitted).  For an η fitted per patch, or
by the plain fitmixtureGP! with a kernel that carries no closure."""
function querymixtureGP!(Yq::Vector{T}, Vq::Vector{T}, Xq::Vector{Vector{T}}, η::MixtureGPType{T}, root, levels,
                         radius::T, δ::T, weight_θ)::Nothing where T
    η.model == C_NULL && throw(PMKError("fitmixtureGP! must run before querymixtureGP!"))
    Nq = length(Xq); Xm = array2matrix(Xq)
    resize!(Yq, Nq); resize!(Vq, Nq)
    check(ccall((:pmk_model_set_bsp, libpmk), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Int64), η.model, native(root), 0), "pmk_model_set_bsp")
    check(ccall((:pmk_predict_mixture_fitted, libpmk), Cint,
                (Ptr{Cvoid}, Ref{KernelDesc}, Int64, Ptr{Float64}, Float64, Float64, Ptr{Float64}, Ptr{Float64}),
                η.model, Ref(desc(weight_θ)), Nq, Xm, radius, δ, Yq, Vq), "pmk_predict_mixture_fitted")
    return nothing
end

"""querymixtureGPmulti!(Yq, Vq, Xq, η, root, levels, radius, δ, weight_θ): the same for R target columns solved on the
resident per-patch factor (pmk_predict_mixture_multi_fitted); Vq === nothing skips the variance."""
function querymixtureGPmulti!(Yq::Matrix{T}, Vq::Union{Vector{T},Nothing}, Xq::Vector{Vector{T}}, η::MixtureGPType{T}, root,
                              levels, radius::T, δ::T, weight_θ)::Nothing where T
    η.model == C_NULL && throw(PMKError("fitmixtureGP! must run before querymixtureGPmulti!"))
    Nq = length(Xq); Xm = array2matrix(Xq)
    size(Yq, 1) == Nq && 1 <= size(Yq, 2) <= 16 || throw(ArgumentError("Yq must be length(Xq) x R"))
    Ym = Matrix{Float64}(undef, Nq, 16)
    Vq === nothing || resize!(Vq, Nq)
    check(ccall((:pmk_model_set_bsp, libpmk), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Int64), η.model, native(root), 0), "pmk_model_set_bsp")
    check(ccall((:pmk_predict_mixture_multi_fitted, libpmk), Cint,
                (Ptr{Cvoid}, Ref{KernelDesc}, Int64, Ptr{Float64}, Float64, Float64, Ptr{Float64}, Int64, Ptr{Float64}),
                η.model, Ref(desc(weight_θ)), Nq, Xm, radius, δ, Ym, max(Nq, 1),
                Vq === nothing ? Ptr{Float64}(C_NULL) : pointer(Vq)), "pmk_predict_mixture_multi_fitted")
    Yq .= view(Ym, :, 1:size(Yq, 2))
    return nothing
end

"""querymixtureGP_grad(Xq, η, root, levels, radius, δ, weight_θ; items = false) -> (Yq, dYq): the blended mean of the R
target columns (Nq x R) and its gradient, dYq[j, d, c] = ∂Y_c/∂x_d at query j (Nq x D x R), with the model's own kernels
and its trend if one is set (pmk_predict_mixture_grad_fitted).  The derivative holds the item list of each query fixed:
where that list changes (the radius cut-off, a δ test, a change of home leaf) the blend itself jumps.  Brownian-bridge
kernels are refused.  items = true runs the staged calls and also returns (G, plane): G is D x R x total, the per-item
gradients in the item order of the plan, plane the 1-based pre-order hyperplane of every neighbour item (0 for home)."""
function querymixtureGP_grad(Xq::Vector{Vector{Float64}}, η::MixtureGPType{Float64}, root, levels, radius::Float64, δ::Float64,
                             weight_θ; items::Bool = false)
    η.model == C_NULL && throw(PMKError("fitmixtureGPmulti! must run before querymixtureGP_grad"))
    R = η.R_multi
    R >= 1 || throw(PMKError("fitmixtureGPmulti! must run before querymixtureGP_grad"))
    Nq = length(Xq); Xm = array2matrix(Xq); D = size(Xm, 1)
    Yq = Matrix{Float64}(undef, Nq, R); dYq = Array{Float64,3}(undef, Nq, D, R)
    check(ccall((:pmk_model_set_bsp, libpmk), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Int64), η.model, native(root), 0), "pmk_model_set_bsp")
    if !items
        check(ccall((:pmk_predict_mixture_grad_fitted, libpmk), Cint,
                    (Ptr{Cvoid}, Ref{KernelDesc}, Int64, Ptr{Float64}, Float64, Float64, Ptr{Float64}, Int64, Ptr{Float64}, Int64),
                    η.model, Ref(desc(weight_θ)), Nq, Xm, radius, δ, Yq, max(Nq, 1), dYq, max(Nq, 1)),
              "pmk_predict_mixture_grad_fitted")
        return Yq, dYq
    end
    q = Ref{Ptr{Cvoid}}(C_NULL); total = Ref{Int64}(0)
    check(ccall((:pmk_query_create, libpmk), Cint, (Ptr{Cvoid}, Int64, Ptr{Float64}, Ref{Ptr{Cvoid}}), η.model, Nq, Xm, q), "pmk_query_create")
    try
        check(ccall((:pmk_query_plan, libpmk), Cint, (Ptr{Cvoid}, Float64, Float64), q[], radius, δ), "pmk_query_plan")
        check(ccall((:pmk_query_counts, libpmk), Cint, (Ptr{Cvoid}, Ref{Int64}, Ptr{Int64}, Ptr{Int64}), q[], total,
                    Ptr{Int64}(C_NULL), Ptr{Int64}(C_NULL)), "pmk_query_counts")
        check(ccall((:pmk_query_items_multi_fitted, libpmk), Cint, (Ptr{Cvoid}, Cint), q[], 0), "pmk_query_items_multi_fitted")
        check(ccall((:pmk_query_items_grad, libpmk), Cint, (Ptr{Cvoid}, Ptr{KernelDesc}), q[], Ptr{KernelDesc}(C_NULL)),
              "pmk_query_items_grad")
        check(ccall((:pmk_query_mix_multi, libpmk), Cint, (Ptr{Cvoid}, Ref{KernelDesc}, Int64, Int64), q[], Ref(desc(weight_θ)), 0, Nq),
              "pmk_query_mix_multi")
        check(ccall((:pmk_query_mix_grad, libpmk), Cint, (Ptr{Cvoid}, Ref{KernelDesc}, Int64, Int64), q[], Ref(desc(weight_θ)), 0, Nq),
              "pmk_query_mix_grad")
        check(ccall((:pmk_query_fetch_multi, libpmk), Cint, (Ptr{Cvoid}, Ptr{Float64}, Int64, Ptr{Float64}), q[], Yq, max(Nq, 1),
                    Ptr{Float64}(C_NULL)), "pmk_query_fetch_multi")
        check(ccall((:pmk_query_fetch_grad, libpmk), Cint, (Ptr{Cvoid}, Ptr{Float64}, Int64), q[], dYq, max(Nq, 1)), "pmk_query_fetch_grad")
        G = Array{Float64,3}(undef, D, R, total[]); plane = Vector{Int32}(undef, total[])
        check(ccall((:pmk_query_get_items_grad, libpmk), Cint, (Ptr{Cvoid}, Ptr{Float64}, Int64, Ptr{Int32}), q[], G, D * R, plane),
              "pmk_query_get_items_grad")
        return Yq, dYq, G, Int.(plane) .+ 1
    finally
        ccall((:pmk_query_destroy, libpmk), Cvoid, (Ptr{Cvoid},), q[])
    end
end

"""querymixtureGP_vgrad(Xq, η, root, levels, radius, δ, weight_θ; items = false) -> (Yq, Vq, dYq, dVq): querymixtureGP_grad's
blended means and their gradient, the blended variance Vq (Nq) and its gradient dVq[j, d] = ∂Vq/∂x_d at query j (Nq x D),
with the model's own kernels and its trend if one is set (pmk_predict_mixture_vgrad_fitted).  The derivative holds the item
list of each query fixed.  Brownian-bridge kernels are refused.  items = true runs the staged calls and also returns GV,
D x total: the per-item variance gradients in the item order of the plan."""
function querymixtureGP_vgrad(Xq::Vector{Vector{Float64}}, η::MixtureGPType{Float64}, root, levels, radius::Float64, δ::Float64,
                              weight_θ; items::Bool = false)
    η.model == C_NULL && throw(PMKError("fitmixtureGPmulti! must run before querymixtureGP_vgrad"))
    R = η.R_multi
    R >= 1 || throw(PMKError("fitmixtureGPmulti! must run before querymixtureGP_vgrad"))
    Nq = length(Xq); Xm = array2matrix(Xq); D = size(Xm, 1)
    Yq = Matrix{Float64}(undef, Nq, R); dYq = Array{Float64,3}(undef, Nq, D, R)
    Vq = Vector{Float64}(undef, Nq); dVq = Matrix{Float64}(undef, Nq, D)
    check(ccall((:pmk_model_set_bsp, libpmk), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Int64), η.model, native(root), 0), "pmk_model_set_bsp")
    if !items
        check(ccall((:pmk_predict_mixture_vgrad_fitted, libpmk), Cint,
                    (Ptr{Cvoid}, Ref{KernelDesc}, Int64, Ptr{Float64}, Float64, Float64, Ptr{Float64}, Int64, Ptr{Float64},
                     Ptr{Float64}, Int64, Ptr{Float64}, Int64),
                    η.model, Ref(desc(weight_θ)), Nq, Xm, radius, δ, Yq, max(Nq, 1), Vq, dYq, max(Nq, 1), dVq, max(Nq, 1)),
              "pmk_predict_mixture_vgrad_fitted")
        return Yq, Vq, dYq, dVq
    end
    q = Ref{Ptr{Cvoid}}(C_NULL); total = Ref{Int64}(0)
    check(ccall((:pmk_query_create, libpmk), Cint, (Ptr{Cvoid}, Int64, Ptr{Float64}, Ref{Ptr{Cvoid}}), η.model, Nq, Xm, q), "pmk_query_create")
    try
        check(ccall((:pmk_query_plan, libpmk), Cint, (Ptr{Cvoid}, Float64, Float64), q[], radius, δ), "pmk_query_plan")
        check(ccall((:pmk_query_counts, libpmk), Cint, (Ptr{Cvoid}, Ref{Int64}, Ptr{Int64}, Ptr{Int64}), q[], total,
                    Ptr{Int64}(C_NULL), Ptr{Int64}(C_NULL)), "pmk_query_counts")
        check(ccall((:pmk_query_items_multi_fitted, libpmk), Cint, (Ptr{Cvoid}, Cint), q[], 1), "pmk_query_items_multi_fitted")
        check(ccall((:pmk_query_items_grad, libpmk), Cint, (Ptr{Cvoid}, Ptr{KernelDesc}), q[], Ptr{KernelDesc}(C_NULL)),
              "pmk_query_items_grad")
        check(ccall((:pmk_query_items_vgrad, libpmk), Cint, (Ptr{Cvoid}, Ptr{KernelDesc}), q[], Ptr{KernelDesc}(C_NULL)),
              "pmk_query_items_vgrad")
        check(ccall((:pmk_query_mix_multi, libpmk), Cint, (Ptr{Cvoid}, Ref{KernelDesc}, Int64, Int64), q[], Ref(desc(weight_θ)), 0, Nq),
              "pmk_query_mix_multi")
        check(ccall((:pmk_query_mix_grad, libpmk), Cint, (Ptr{Cvoid}, Ref{KernelDesc}, Int64, Int64), q[], Ref(desc(weight_θ)), 0, Nq),
              "pmk_query_mix_grad")
        check(ccall((:pmk_query_mix_vgrad, libpmk), Cint, (Ptr{Cvoid}, Ref{KernelDesc}, Int64, Int64), q[], Ref(desc(weight_θ)), 0, Nq),
              "pmk_query_mix_vgrad")
        check(ccall((:pmk_query_fetch_multi, libpmk), Cint, (Ptr{Cvoid}, Ptr{Float64}, Int64, Ptr{Float64}), q[], Yq, max(Nq, 1), Vq),
              "pmk_query_fetch_multi")
        check(ccall((:pmk_query_fetch_grad, libpmk), Cint, (Ptr{Cvoid}, Ptr{Float64}, Int64), q[], dYq, max(Nq, 1)), "pmk_query_fetch_grad")
        check(ccall((:pmk_query_fetch_vgrad, libpmk), Cint, (Ptr{Cvoid}, Ptr{Float64}, Int64), q[], dVq, max(Nq, 1)), "pmk_query_fetch_vgrad")
        GV = Matrix{Float64}(undef, D, total[])
        check(ccall((:pmk_query_get_items_vgrad, libpmk), Cint, (Ptr{Cvoid}, Ptr{Float64}, Int64), q[], GV, D), "pmk_query_get_items_vgrad")
        return Yq, Vq, dYq, dVq, GV
    finally
        ccall((:pmk_query_destroy, libpmk), Cvoid, (Ptr{Cvoid},), q[])
    end
end

"""querymixtureGP_cov(Xq, η, root, levels, radius, δ, weight_θ; region = 0, device = C_NULL) -> (Yq, Vq, Cov): the blended
mean and variance of querymixtureGP with the model's own kernels and the joint posterior covariance Cov (Nq x Nq, symmetric)
of the batch under the blend (pmk_predict_mixture_cov_fitted).  Queries that share no region have covariance exactly 0.
Single-output path, no trend; at most 16384 queries.  region = r > 0 runs the staged calls and also returns (query, S): the
posterior covariance block of region r over its items and the 1-based query index of each of its rows.  device: a device
pointer to Nq x Nq Float64 that receives Cov as well (pmk_query_fetch_cov_dev; staged calls)."""
function querymixtureGP_cov(Xq::Vector{Vector{Float64}}, η::MixtureGPType{Float64}, root, levels, radius::Float64, δ::Float64,
                            weight_θ; region::Int = 0, device::Ptr{Float64} = Ptr{Float64}(C_NULL))
    η.model == C_NULL && throw(PMKError("fitmixtureGP! must run before querymixtureGP_cov"))
    Nq = length(Xq); Xm = array2matrix(Xq)
    Yq = Vector{Float64}(undef, Nq); Vq = Vector{Float64}(undef, Nq); Cov = Matrix{Float64}(undef, Nq, Nq)
    check(ccall((:pmk_model_set_bsp, libpmk), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Int64), η.model, native(root), 0), "pmk_model_set_bsp")
    if region == 0 && device == C_NULL
        check(ccall((:pmk_predict_mixture_cov_fitted, libpmk), Cint,
                    (Ptr{Cvoid}, Ref{KernelDesc}, Int64, Ptr{Float64}, Float64, Float64, Ptr{Float64}, Ptr{Float64},
                     Ptr{Float64}, Int64),
                    η.model, Ref(desc(weight_θ)), Nq, Xm, radius, δ, Yq, Vq, Cov, max(Nq, 1)),
              "pmk_predict_mixture_cov_fitted")
        return Yq, Vq, Cov
    end
    q = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:pmk_query_create, libpmk), Cint, (Ptr{Cvoid}, Int64, Ptr{Float64}, Ref{Ptr{Cvoid}}), η.model, Nq, Xm, q), "pmk_query_create")
    try
        check(ccall((:pmk_query_plan, libpmk), Cint, (Ptr{Cvoid}, Float64, Float64), q[], radius, δ), "pmk_query_plan")
        check(ccall((:pmk_query_items_fitted, libpmk), Cint, (Ptr{Cvoid},), q[]), "pmk_query_items_fitted")
        check(ccall((:pmk_query_mix, libpmk), Cint, (Ptr{Cvoid}, Ref{KernelDesc}, Int64, Int64), q[], Ref(desc(weight_θ)), 0, Nq),
              "pmk_query_mix")
        check(ccall((:pmk_query_items_cov, libpmk), Cint, (Ptr{Cvoid}, Ptr{KernelDesc}), q[], Ptr{KernelDesc}(C_NULL)),
              "pmk_query_items_cov")
        check(ccall((:pmk_query_mix_cov, libpmk), Cint, (Ptr{Cvoid}, Ref{KernelDesc}), q[], Ref(desc(weight_θ))), "pmk_query_mix_cov")
        check(ccall((:pmk_query_fetch, libpmk), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}), q[], Yq, Vq), "pmk_query_fetch")
        check(ccall((:pmk_query_fetch_cov, libpmk), Cint, (Ptr{Cvoid}, Ptr{Float64}, Int64), q[], Cov, max(Nq, 1)), "pmk_query_fetch_cov")
        if device != C_NULL
            check(ccall((:pmk_query_fetch_cov_dev, libpmk), Cint, (Ptr{Cvoid}, Ptr{Float64}, Int64), q[], device, max(Nq, 1)),
                  "pmk_query_fetch_cov_dev")
        end
        region == 0 && return Yq, Vq, Cov
        m = Ref{Int64}(0)
        check(ccall((:pmk_query_get_items_cov, libpmk), Cint, (Ptr{Cvoid}, Int64, Ref{Int64}, Ptr{Int32}, Ptr{Float64}, Int64),
                    q[], region - 1, m, Ptr{Int32}(C_NULL), Ptr{Float64}(C_NULL), 0), "pmk_query_get_items_cov")
        query = Vector{Int32}(undef, m[]); S = Matrix{Float64}(undef, m[], m[])
        check(ccall((:pmk_query_get_items_cov, libpmk), Cint, (Ptr{Cvoid}, Int64, Ptr{Int64}, Ptr{Int32}, Ptr{Float64}, Int64),
                    q[], region - 1, Ptr{Int64}(C_NULL), query, S, max(m[], 1)), "pmk_query_get_items_cov")
        return Yq, Vq, Cov, query .+ Int32(1), S
    finally
        ccall((:pmk_query_destroy, libpmk), Cvoid, (Ptr{Cvoid},), q[])
    end
end

"""querymixtureGP_cov_multi(Xq, η, root, levels, radius, δ, weight_θ; staged = false) -> (Yq, Vq, Cov): the R blended means
(Nq x R) and the variance of querymixtureGPmulti! with the model's own kernels, and the joint posterior covariance Cov
(Nq x Nq, symmetric) of the batch, for the columns of fitmixtureGPmulti! with the trend of settrendmixtureGP! if one is set
(pmk_predict_mixture_cov_multi_fitted).  Under a trend Cov is the universal-kriging covariance and its diagonal is Vq up to
rounding; the R columns are independent fields and share it.  staged = true runs the staged calls instead
(pmk_query_items_cov_multi); the results are the same.  At most 16384 queries."""
function querymixtureGP_cov_multi(Xq::Vector{Vector{Float64}}, η::MixtureGPType{Float64}, root, levels, radius::Float64,
                                  δ::Float64, weight_θ; staged::Bool = false)
    η.model == C_NULL && throw(PMKError("fitmixtureGPmulti! must run before querymixtureGP_cov_multi"))
    R = η.R_multi
    R >= 1 || throw(PMKError("fitmixtureGPmulti! must run before querymixtureGP_cov_multi"))
    Nq = length(Xq); Xm = array2matrix(Xq)
    Yq = Matrix{Float64}(undef, Nq, R); Vq = Vector{Float64}(undef, Nq); Cov = Matrix{Float64}(undef, Nq, Nq)
    check(ccall((:pmk_model_set_bsp, libpmk), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Int64), η.model, native(root), 0), "pmk_model_set_bsp")
    if !staged
        check(ccall((:pmk_predict_mixture_cov_multi_fitted, libpmk), Cint,
                    (Ptr{Cvoid}, Ref{KernelDesc}, Int64, Ptr{Float64}, Float64, Float64, Ptr{Float64}, Int64, Ptr{Float64},
                     Ptr{Float64}, Int64),
                    η.model, Ref(desc(weight_θ)), Nq, Xm, radius, δ, Yq, max(Nq, 1), Vq, Cov, max(Nq, 1)),
              "pmk_predict_mixture_cov_multi_fitted")
        return Yq, Vq, Cov
    end
    q = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:pmk_query_create, libpmk), Cint, (Ptr{Cvoid}, Int64, Ptr{Float64}, Ref{Ptr{Cvoid}}), η.model, Nq, Xm, q), "pmk_query_create")
    try
        check(ccall((:pmk_query_plan, libpmk), Cint, (Ptr{Cvoid}, Float64, Float64), q[], radius, δ), "pmk_query_plan")
        check(ccall((:pmk_query_items_multi_fitted, libpmk), Cint, (Ptr{Cvoid}, Cint), q[], 1), "pmk_query_items_multi_fitted")
        check(ccall((:pmk_query_mix_multi, libpmk), Cint, (Ptr{Cvoid}, Ref{KernelDesc}, Int64, Int64), q[], Ref(desc(weight_θ)), 0, Nq),
              "pmk_query_mix_multi")
        check(ccall((:pmk_query_items_cov_multi, libpmk), Cint, (Ptr{Cvoid}, Ptr{KernelDesc}), q[], Ptr{KernelDesc}(C_NULL)),
              "pmk_query_items_cov_multi")
        check(ccall((:pmk_query_mix_cov, libpmk), Cint, (Ptr{Cvoid}, Ref{KernelDesc}), q[], Ref(desc(weight_θ))), "pmk_query_mix_cov")
        check(ccall((:pmk_query_fetch_multi, libpmk), Cint, (Ptr{Cvoid}, Ptr{Float64}, Int64, Ptr{Float64}), q[], Yq, max(Nq, 1), Vq),
              "pmk_query_fetch_multi")
        check(ccall((:pmk_query_fetch_cov, libpmk), Cint, (Ptr{Cvoid}, Ptr{Float64}, Int64), q[], Cov, max(Nq, 1)), "pmk_query_fetch_cov")
        return Yq, Vq, Cov
    finally
        ccall((:pmk_query_destroy, libpmk), Cvoid, (Ptr{Cvoid},), q[])
    end
end

"""querymixtureGP_block(Xq, group, a, η, root, levels, radius, δ, weight_θ; variance = true, staged = false) -> (Yb, Vb):
block kriging (change of support).  Yb (F x R) is the prediction of sum_j a[j] f(x_j) over the queries j of every group and
Vb (F) its kriging variance, for the columns of fitmixtureGPmulti! with the trend of settrendmixtureGP! if one is set
(pmk_predict_mixture_block_fitted).  group[j] in 1:F is NON-DECREASING in j: the queries of a group are contiguous, a group
may be empty; F = group[end].  a[j] is any real.  Vb is a' Cov a of querymixtureGP_cov_multi without the Nq x Nq matrix and
without its limit of 16384 queries.  variance = false returns (Yb, nothing).  staged = true runs the staged calls
(pmk_query_items_block); the results are the same."""
function querymixtureGP_block(Xq::Vector{Vector{Float64}}, group::Vector{<:Integer}, a::Vector{Float64},
                              η::MixtureGPType{Float64}, root, levels, radius::Float64, δ::Float64, weight_θ;
                              variance::Bool = true, staged::Bool = false)
    η.model == C_NULL && throw(PMKError("fitmixtureGPmulti! must run before querymixtureGP_block"))
    R = η.R_multi
    R >= 1 || throw(PMKError("fitmixtureGPmulti! must run before querymixtureGP_block"))
    Nq = length(Xq); Xm = array2matrix(Xq)
    (length(group) == Nq && length(a) == Nq) || throw(ArgumentError("one group and one coefficient per query point"))
    g0 = Int32.(group .- 1)
    F = Nq == 0 ? 0 : Int(group[end])
    Yb = Matrix{Float64}(undef, F, R); Vb = Vector{Float64}(undef, F)
    vptr = variance ? pointer(Vb) : Ptr{Float64}(C_NULL)
    check(ccall((:pmk_model_set_bsp, libpmk), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Int64), η.model, native(root), 0), "pmk_model_set_bsp")
    if !staged
        GC.@preserve Vb check(ccall((:pmk_predict_mixture_block_fitted, libpmk), Cint,
                    (Ptr{Cvoid}, Ref{KernelDesc}, Int64, Ptr{Float64}, Float64, Float64, Int64, Ptr{Int32}, Ptr{Float64},
                     Ptr{Float64}, Int64, Ptr{Float64}),
                    η.model, Ref(desc(weight_θ)), Nq, Xm, radius, δ, F, g0, a, Yb, max(F, 1), vptr),
              "pmk_predict_mixture_block_fitted")
        return Yb, (variance ? Vb : nothing)
    end
    q = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:pmk_query_create, libpmk), Cint, (Ptr{Cvoid}, Int64, Ptr{Float64}, Ref{Ptr{Cvoid}}), η.model, Nq, Xm, q), "pmk_query_create")
    try
        check(ccall((:pmk_query_plan, libpmk), Cint, (Ptr{Cvoid}, Float64, Float64), q[], radius, δ), "pmk_query_plan")
        check(ccall((:pmk_query_items_multi_fitted, libpmk), Cint, (Ptr{Cvoid}, Cint), q[], 0), "pmk_query_items_multi_fitted")
        check(ccall((:pmk_query_items_block, libpmk), Cint,
                    (Ptr{Cvoid}, Ptr{KernelDesc}, Ref{KernelDesc}, Int64, Ptr{Int32}, Ptr{Float64}, Cint),
                    q[], Ptr{KernelDesc}(C_NULL), Ref(desc(weight_θ)), F, g0, a, variance ? 1 : 0), "pmk_query_items_block")
        GC.@preserve Vb check(ccall((:pmk_query_fetch_block, libpmk), Cint, (Ptr{Cvoid}, Ptr{Float64}, Int64, Ptr{Float64}),
                    q[], Yb, max(F, 1), vptr), "pmk_query_fetch_block")
        return Yb, (variance ? Vb : nothing)
    finally
        ccall((:pmk_query_destroy, libpmk), Cvoid, (Ptr{Cvoid},), q[])
    end
end

"""samplemixtureGP_blocks(Xq, η, root, levels, radius, δ, weight_θ, Z; multi = false, region = 0) -> (E, jitter, total): the zero-mean
part E (Nq x n) of n joint posterior draws of the blended field from the region blocks, without the Nq x Nq covariance
(pmk_query_items_cov_blocks, pmk_query_factor_cov, pmk_query_draw): Nq may exceed 16384.  Z (ldz x n, ldz >= total) holds
independent standard normals, column s for draw s, row p for the sorted item p; since total depends on the plan, a call
with Z = zeros(0, 0) returns (zeros(Nq, 0), 0.0, total) and draws nothing.  The caller adds the blended mean; for R target
columns (multi = true, after fitmixtureGPmulti!) one call per column with independent Z.  The jitter ladder runs per region:
rel = 0, then for the failed regions 2^-52 and x 10 while rel <= 2^-26, on the scale trace S_r / m_r; jitter is the largest
absolute value added.  Throws if a region that holds items belongs to a failed patch or cannot be factored.  region = r > 0
also returns L_r, the lower-triangular factor of the block of region r (pmk_query_get_items_cov_factor)."""
function samplemixtureGP_blocks(Xq::Vector{Vector{Float64}}, η::MixtureGPType{Float64}, root, levels, radius::Float64,
                                δ::Float64, weight_θ, Z::Matrix{Float64}; multi::Bool = false, region::Int = 0)
    η.model == C_NULL && throw(PMKError("fitmixtureGP! must run before samplemixtureGP_blocks"))
    Nq = length(Xq); Xm = array2matrix(Xq)
    check(ccall((:pmk_model_set_bsp, libpmk), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Int64), η.model, native(root), 0), "pmk_model_set_bsp")
    P = Int(ccall((:pmk_model_num_patches, libpmk), Int64, (Ptr{Cvoid},), η.model))
    q = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:pmk_query_create, libpmk), Cint, (Ptr{Cvoid}, Int64, Ptr{Float64}, Ref{Ptr{Cvoid}}), η.model, Nq, Xm, q), "pmk_query_create")
    try
        check(ccall((:pmk_query_plan, libpmk), Cint, (Ptr{Cvoid}, Float64, Float64), q[], radius, δ), "pmk_query_plan")
        total = Ref{Int64}(0)
        check(ccall((:pmk_query_counts, libpmk), Cint, (Ptr{Cvoid}, Ref{Int64}, Ptr{Int64}, Ptr{Int64}), q[], total,
                    Ptr{Int64}(C_NULL), Ptr{Int64}(C_NULL)), "pmk_query_counts")
        size(Z, 2) == 0 && return zeros(Nq, 0), 0.0, Int(total[])
        size(Z, 1) >= total[] || throw(PMKError("Z has $(size(Z, 1)) rows, the plan $(total[]) items"))
        if multi
            check(ccall((:pmk_query_items_multi_fitted, libpmk), Cint, (Ptr{Cvoid}, Cint), q[], 1), "pmk_query_items_multi_fitted")
        else
            check(ccall((:pmk_query_items_fitted, libpmk), Cint, (Ptr{Cvoid},), q[]), "pmk_query_items_fitted")
        end
        check(ccall((:pmk_query_items_cov_blocks, libpmk), Cint, (Ptr{Cvoid}, Ptr{KernelDesc}, Cint), q[], Ptr{KernelDesc}(C_NULL),
                    multi ? 1 : 0), "pmk_query_items_cov_blocks")
        roff = Vector{Int64}(undef, P + 1)
        check(ccall((:pmk_query_region_offsets, libpmk), Cint, (Ptr{Cvoid}, Ptr{Int64}), q[], roff), "pmk_query_region_offsets")
        rel = zeros(P); finfo = Vector{Int32}(undef, P); jit = Vector{Float64}(undef, P)
        while true
            check(ccall((:pmk_query_factor_cov, libpmk), Cint, (Ptr{Cvoid}, Ptr{Float64}), q[], rel), "pmk_query_factor_cov")
            check(ccall((:pmk_query_factor_info, libpmk), Cint, (Ptr{Cvoid}, Ptr{Int32}, Ptr{Float64}), q[], finfo, jit),
                  "pmk_query_factor_info")
            for r = 1:P
                finfo[r] == -1 && roff[r + 1] > roff[r] &&
                    throw(PMKError("samplemixtureGP_blocks: region $r holds items of the batch and its patch is failed"))
            end
            failed = findall(>(0), finfo)
            isempty(failed) && break
            for r in failed
                rel[r] = rel[r] == 0.0 ? 2.0^-52 : 10.0 * rel[r]
                rel[r] <= 2.0^-26 || throw(PMKError("samplemixtureGP_blocks: the block of region $r is not positive definite " *
                                                    "with a jitter of up to 2^-26 trace / m"))
            end
        end
        n = size(Z, 2)
        E = Matrix{Float64}(undef, Nq, n)
        check(ccall((:pmk_query_draw, libpmk), Cint, (Ptr{Cvoid}, Ref{KernelDesc}, Int64, Ptr{Float64}, Int64, Ptr{Float64}, Int64),
                    q[], Ref(desc(weight_θ)), n, Z, size(Z, 1), E, max(Nq, 1)), "pmk_query_draw")
        jitter = P > 0 ? maximum(jit) : 0.0
        region == 0 && return E, jitter, Int(total[])
        m = Ref{Int64}(0)
        check(ccall((:pmk_query_get_items_cov_factor, libpmk), Cint, (Ptr{Cvoid}, Int64, Ref{Int64}, Ptr{Float64}, Int64),
                    q[], region - 1, m, Ptr{Float64}(C_NULL), 0), "pmk_query_get_items_cov_factor")
        L = Matrix{Float64}(undef, m[], m[])
        check(ccall((:pmk_query_get_items_cov_factor, libpmk), Cint, (Ptr{Cvoid}, Int64, Ptr{Int64}, Ptr{Float64}, Int64),
                    q[], region - 1, Ptr{Int64}(C_NULL), L, max(m[], 1)), "pmk_query_get_items_cov_factor")
        return E, jitter, Int(total[]), L
    finally
        ccall((:pmk_query_destroy, libpmk), Cvoid, (Ptr{Cvoid},), q[])
    end
end

"""selectcandidates(scores) -> winners: per column (patch) of the G x P score matrix the row of the highest score; ties
go to the lowest row, a NaN never wins, and a patch whose scores are all NaN throws, naming the patch."""
function selectcandidates(scores::Matrix{Float64})::Vector{Int}
    G, P = size(scores)
    winners = Vector{Int}(undef, P)
    for r = 1:P
        best = 0
        for g = 1:G
            isnan(scores[g, r]) && continue
            (best == 0 || scores[g, r] > scores[best, r]) && (best = g)
        end
        best == 0 && throw(ArgumentError("patch $r: every candidate scored NaN (no candidate could be factorised)"))
        winners[r] = best
    end
    return winners
end

"""selectmixtureGP!(η, y_parts, candidates; score = :evidence) -> (η, winners, scores): `candidates` is a vector of
(θ, σ²).  Every candidate is fitted uniformly (pmk_model_fit) and scored per patch: :evidence is the log marginal
likelihood of logevidencemixtureGP, :loo the leave-one-out log pseudo-likelihood
Σᵢ [-½ log varᵢ - resᵢ² / (2 varᵢ) - ½ log 2π] (Rasmussen & Williams eq. 5.10-5.11) from pmk_model_loo.  A patch whose
factorisation fails under a candidate scores NaN for it.  selectcandidates picks the winners and one per-patch fit with
them leaves η fitted.  Cost: G fits (plus G leave-one-out passes for :loo) plus one fit."""
function selectmixtureGP!(η::MixtureGPType{T}, y_parts::Vector{Vector{T}}, candidates::Vector; score::Symbol = :evidence) where T
    score in (:evidence, :loo) || throw(ArgumentError("score must be :evidence or :loo"))
    G = length(candidates); P = length(η.X_parts)
    G >= 1 || throw(ArgumentError("no candidates"))
    all(c -> perpatchok(c[1]), candidates) || throw(ArgumentError("closure-carrying kernels cannot be set per patch"))
    Xm = [array2matrix(X) for X in η.X_parts]; ys = [Vector{Float64}(y) for y in y_parts]
    n = Int64[size(x, 2) for x in Xm]; D = size(Xm[1], 1)
    h = Ref{Ptr{Cvoid}}(C_NULL); info = Vector{Int32}(undef, P)
    GC.@preserve Xm ys begin
        check(ccall((:pmk_model_create, libpmk), Cint,
            (Ptr{Cvoid}, Cint, Int64, Ptr{Int64}, Ptr{Ptr{Float64}}, Ptr{Ptr{Float64}}, Ref{Ptr{Cvoid}}),
            context(), D, P, n, [pointer(x) for x in Xm], [pointer(y) for y in ys], h), "pmk_model_create")
    end
    scores = Matrix{Float64}(undef, G, P)
    logdet = Vector{Float64}(undef, P); quad = Vector{Float64}(undef, P)
    res = [Vector{Float64}(undef, Int(n[r])) for r = 1:P]; var = [Vector{Float64}(undef, Int(n[r])) for r = 1:P]
    try
        for g = 1:G
            θ, σ² = candidates[g]
            check(ccall((:pmk_model_fit, libpmk), Cint, (Ptr{Cvoid}, Ref{KernelDesc}, Float64), h[], Ref(desc(θ)), σ²), "pmk_model_fit")
            check(ccall((:pmk_model_info, libpmk), Cint, (Ptr{Cvoid}, Ptr{Int32}), h[], info), "pmk_model_info")
            if score == :evidence
                check(ccall((:pmk_model_evidence, libpmk), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}), h[], logdet, quad),
                      "pmk_model_evidence")
                scores[g, :] = [-0.5 * quad[r] - 0.5 * logdet[r] - 0.5 * n[r] * log(2π) for r = 1:P]
            else
                check(ccall((:pmk_model_loo, libpmk), Cint, (Ptr{Cvoid},), h[]), "pmk_model_loo")
                GC.@preserve res var check(ccall((:pmk_model_get_loo, libpmk), Cint, (Ptr{Cvoid}, Ptr{Ptr{Float64}}, Ptr{Ptr{Float64}}),
                                                 h[], [pointer(a) for a in res], [pointer(a) for a in var]), "pmk_model_get_loo")
                scores[g, :] = [sum(-0.5 .* log.(var[r]) .- res[r] .^ 2 ./ (2 .* var[r]) .- 0.5 * log(2π)) for r = 1:P]
            end
        end
    finally
        ccall((:pmk_model_destroy, libpmk), Cvoid, (Ptr{Cvoid},), h[])
    end
    winners = selectcandidates(scores)
    fitmixtureGP!(η, y_parts, Any[candidates[w][1] for w in winners], Float64[candidates[w][2] for w in winners])
    return η, winners, scores
end

# ------------------------------------------------------------------------------------------ multi-GPU (one process per GPU)
"""Comm(rank, world, id): the library's own RCCL communicator (pmk_comm_create; collective).  Rank 0 makes `id` with
`comm_unique_id()` and ships the 128 bytes to the other ranks by any host channel (MPI.jl's `MPI.Bcast!`, a file ...)."""
mutable struct Comm
    h::Ptr{Cvoid}
    rank::Int
    world::Int
end
function comm_unique_id()
    id = Vector{UInt8}(undef, 128)
    check(ccall((:pmk_comm_unique_id, libpmk), Cint, (Ptr{UInt8},), id), "pmk_comm_unique_id")
    return id
end
function Comm(rank::Integer, world::Integer, id::Vector{UInt8})
    h = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:pmk_comm_create, libpmk), Cint, (Ptr{Cvoid}, Cint, Cint, Ptr{UInt8}, Ref{Ptr{Cvoid}}),
                context(), rank, world, id, h), "pmk_comm_create")
    c = Comm(h[], rank, world)
    finalizer(x -> (ccall((:pmk_comm_destroy, libpmk), Cvoid, (Ptr{Cvoid},), x.h); nothing), c)
    return c
end

"""querymixtureGP!(Yq, Vq, Xq_local, η_local, comm, root, levels, radius, δ, θ, σ², weight_θ): the sharded form of
querymixtureGP! (mixtureGP.jl:159-294).  This rank's `η_local` holds the leaves `rank*P/world+1 : (rank+1)*P/world` of the
replicated tree `root` (fit them with fitmixtureGP! on `X_set[that range]`), `Xq_local` is this rank's share of the
queries; requests travel to the leaf owners and (u, v) back over RCCL inside the library (pmk_query_predict_sharded)."""
function querymixtureGP!(Yq::Vector{T}, Vq::Vector{T}, Xq::Vector{Vector{T}}, η::MixtureGPType{T}, comm::Comm, root, levels,
                         radius::T, δ::T, θ, σ², weight_θ)::Nothing where T
    η.model == C_NULL && throw(PMKError("fitmixtureGP! must run before querymixtureGP!"))
    Nq = length(Xq); Xm = pack(Xq)
    resize!(Yq, Nq); resize!(Vq, Nq)
    P = Int(ccall((:pmk_model_num_patches, libpmk), Int64, (Ptr{Cvoid},), η.model))
    check(ccall((:pmk_model_set_bsp, libpmk), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Int64), η.model, native(root), comm.rank * P), "pmk_model_set_bsp")
    q = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:pmk_query_create, libpmk), Cint, (Ptr{Cvoid}, Int64, Ptr{Float64}, Ref{Ptr{Cvoid}}), η.model, Nq, Xm, q), "pmk_query_create")
    try
        check(ccall((:pmk_query_predict_sharded, libpmk), Cint,
            (Ptr{Cvoid}, Ptr{Cvoid}, Ref{KernelDesc}, Ref{KernelDesc}, Float64, Float64, Ptr{Int64}),
            q[], comm.h, Ref(desc(θ)), Ref(desc(weight_θ)), radius, δ, C_NULL), "pmk_query_predict_sharded")
        check(ccall((:pmk_query_fetch, libpmk), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}), q[], Yq, Vq), "pmk_query_fetch")
    finally
        ccall((:pmk_query_destroy, libpmk), Cvoid, (Ptr{Cvoid},), q[])
    end
    return nothing
end

"""querymixtureGP_allgather!(Yq, Vq, Xq_all, η_local, comm, root, levels, radius, δ, θ, σ², weight_θ): the replicated-query form
of the sharded predict step (pmk_query_predict_allgather): every rank passes ALL queries, evaluates the items of its own
leaves, one RCCL all-gather of the (u, v) slices, and every rank ends with all of Yq, Vq."""
function querymixtureGP_allgather!(Yq::Vector{T}, Vq::Vector{T}, Xq::Vector{Vector{T}}, η::MixtureGPType{T}, comm::Comm, root, levels,
                                   radius::T, δ::T, θ, σ², weight_θ)::Nothing where T
    η.model == C_NULL && throw(PMKError("fitmixtureGP! must run before querymixtureGP_allgather!"))
    Nq = length(Xq); Xm = pack(Xq)
    resize!(Yq, Nq); resize!(Vq, Nq)
    P = Int(ccall((:pmk_model_num_patches, libpmk), Int64, (Ptr{Cvoid},), η.model))
    check(ccall((:pmk_model_set_bsp, libpmk), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Int64), η.model, native(root), comm.rank * P), "pmk_model_set_bsp")
    q = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:pmk_query_create, libpmk), Cint, (Ptr{Cvoid}, Int64, Ptr{Float64}, Ref{Ptr{Cvoid}}), η.model, Nq, Xm, q), "pmk_query_create")
    try
        check(ccall((:pmk_query_predict_allgather, libpmk), Cint,
            (Ptr{Cvoid}, Ptr{Cvoid}, Ref{KernelDesc}, Ref{KernelDesc}, Float64, Float64, Ptr{Int64}),
            q[], comm.h, Ref(desc(θ)), Ref(desc(weight_θ)), radius, δ, C_NULL), "pmk_query_predict_allgather")
        check(ccall((:pmk_query_fetch, libpmk), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}), q[], Yq, Vq), "pmk_query_fetch")
    finally
        ccall((:pmk_query_destroy, libpmk), Cvoid, (Ptr{Cvoid},), q[])
    end
    return nothing
end

function querymixtureGP(Xq::Vector{Vector{T}}, η::MixtureGPType{T}, root, levels, radius::T, δ::T, θ, σ², weight_θ;
                        debug_flag = false) where T
    Yq = Vector{T}(undef, 0); Vq = Vector{T}(undef, 0)
    debug_vars = MixtureGPDebugType(one(T))
    querymixtureGP!(Yq, Vq, Xq, η, root, levels, radius, δ, θ, σ², weight_θ, debug_vars; debug_flag = debug_flag)
    return Yq, Vq, debug_vars
end
querymixtureGP(xq::Vector{T}, η::MixtureGPType{T}, root, levels, radius::T, δ::T, θ, σ², weight_θ; debug_flag = false) where T <: Real =
    querymixtureGP([xq], η, root, levels, radius, δ, θ, σ², weight_θ; debug_flag = debug_flag)

"""queryinner(xq, X, θ, c, L) -> (μ, σ²) (mixtureGP.jl:296-320): host factors are uploaded with pmk_model_load and
one strip of the prediction kernel runs against them"""
# the last (X, c, L) that queryinner uploaded, by identity: a loop over query points against one patch (dev/debug.jl:46)
# moves the n x n factor to the device once, not once per point
mutable struct InnerCache
    key::Tuple{UInt,UInt,UInt}
    model::Ptr{Cvoid}
end
const INNER_CACHE = InnerCache((UInt(0), UInt(0), UInt(0)), C_NULL)

function queryinner(xq::Vector{T}, X, θ, c, L) where T
    key = (objectid(X), objectid(c), objectid(L))
    if INNER_CACHE.model == C_NULL || INNER_CACHE.key != key
        if INNER_CACHE.model != C_NULL
            ccall((:pmk_model_destroy, libpmk), Cvoid, (Ptr{Cvoid},), INNER_CACHE.model)
            INNER_CACHE.model = C_NULL
        end
        Xm = pack(X); D, n = size(Xm)
        cc = Vector{Float64}(c); Lm = Matrix{Float64}(L)
        h = Ref{Ptr{Cvoid}}(C_NULL)
        GC.@preserve Xm cc Lm begin
            check(ccall((:pmk_model_load, libpmk), Cint,
                (Ptr{Cvoid}, Cint, Int64, Ptr{Int64}, Ptr{Ptr{Float64}}, Ptr{Ptr{Float64}}, Ptr{Ptr{Float64}}, Ptr{Int64}, Ref{Ptr{Cvoid}}),
                context(), D, 1, Int64[n], [pointer(Xm)], [pointer(cc)], [pointer(Lm)], Int64[n], h), "pmk_model_load")
        end
        INNER_CACHE.model = h[]; INNER_CACHE.key = key
    end
    μ = Ref{Float64}(0.0); v = Ref{Float64}(0.0)
    check(ccall((:pmk_model_queryinner, libpmk), Cint,
        (Ptr{Cvoid}, Int64, Ref{KernelDesc}, Int64, Ptr{Float64}, Ref{Float64}, Ref{Float64}),
        INNER_CACHE.model, 0, Ref(desc(θ)), 1, Vector{Float64}(xq), μ, v), "queryinner")
    return μ[], v[]
end
queryinner!(kq::Vector{T}, xq, X, θ, c, L; min_v = 1e-12) where T = queryinner(xq, X, θ, c, L)

# ------------------------------------------------------------------------------------------ single problem
struct RKHSProblemType{Kernel_Type,T,X_Type}      # src/misc/declarations.jl:226-231
    c::Vector{T}
    X::Vector{X_Type}
    θ::Kernel_Type
    σ²::T
end

"""fitRKHS!(η, y): η.c[:] = (K + σ²I) \\ y (src/RKHS/RKHS.jl:182-217), one patch through the batched fit"""
function fitRKHS!(η, y::Vector{T}) where T
    @assert !isempty(η.X)
    @assert !isempty(y)
    @assert length(η.X) == length(y)
    Xm = kpack(η.θ, η.X); yy = Vector{Float64}(y); D, n = size(Xm)
    h = Ref{Ptr{Cvoid}}(C_NULL); info = Vector{Int32}(undef, 1); c = Vector{Float64}(undef, n); d = Ref(desc(η.θ))
    GC.@preserve Xm yy c begin
        rc = ccall((:pmk_fit_batched, libpmk), Cint,
            (Ptr{Cvoid}, Ref{KernelDesc}, Float64, Cint, Int64, Ptr{Int64}, Ptr{Ptr{Float64}}, Ptr{Ptr{Float64}},
             Ref{Ptr{Cvoid}}, Ptr{Ptr{Float64}}, Ptr{Int32}),
            context(), d, η.σ²[1], D, 1, Int64[n], [pointer(Xm)], [pointer(yy)], h, [pointer(c)], info)
    end
    check(rc, "fitRKHS!")
    ccall((:pmk_model_destroy, libpmk), Cvoid, (Ptr{Cvoid},), h[])
    info[1] == 0 || throw(PosDefException(Int(info[1])))
    η.c[:] = c
    return nothing
end

"""query!(Yq, Xq, η): mean only (src/RKHS/RKHS.jl:220-247)"""
function query!(Yq::Vector{T}, Xq, η::RKHSProblemType) where T
    @assert !isempty(Xq)
    @assert size(Yq) == size(Xq)
    Xm = kpack(η.θ, η.X); Qm = kpack(η.θ, Xq); D, n = size(Xm); Nq = size(Qm, 2)
    out = Vector{Float64}(undef, Nq)
    check(ccall((:pmk_query_mean, libpmk), Cint,
        (Ptr{Cvoid}, Ref{KernelDesc}, Cint, Int64, Ptr{Float64}, Ptr{Float64}, Int64, Ptr{Float64}, Ptr{Float64}),
        context(), Ref(desc(η.θ)), D, n, Xm, Vector{Float64}(η.c), Nq, Qm, out), "query!")
    Yq[:] = out
    return nothing
end

"""query!(Yq, Xq, η::RKHSProblemType{Vector{KT}}) (src/RKHS/RKHS.jl:278-305): one kernel per centre"""
function query!(Yq::Vector{T}, Xq::Vector{Vector{T}}, η::RKHSProblemType{Vector{KT},T}) where {KT,T}
    @assert !isempty(Xq)
    @assert size(Yq) == size(Xq)
    Xm = pack(η.X); Qm = pack(Xq); D, n = size(Xm); Nq = size(Qm, 2)
    @assert length(η.θ) == n
    ds = [desc(θ) for θ in η.θ]
    out = Vector{Float64}(undef, Nq)
    check(ccall((:pmk_query_mean_multi, libpmk), Cint,
        (Ptr{Cvoid}, Ptr{KernelDesc}, Cint, Int64, Ptr{Float64}, Ptr{Float64}, Int64, Ptr{Float64}, Ptr{Float64}),
        context(), ds, D, n, Xm, Vector{Float64}(η.c), Nq, Qm, out), "query!")
    Yq[:] = out
    return nothing
end

"""setupGPquery(c, X, θ, σ²) -> fq, fq(xq) = (mean, variance) (src/RKHS/querying.jl:43-79).  The reference's closure
solves `A \\ k` by LU on every call; here K + σ²I is factorised once on the device and a call is one strip of the
prediction kernel.  The variance is `k(xq,xq) - k'(A \\ k)` as the reference returns it: not clamped."""
function setupGPquery(c::Vector{T}, X, θ, σ²::T)::Function where T
    Xm = kpack(θ, X); D, n = size(Xm)
    @assert length(c) == n
    h = Ref{Ptr{Cvoid}}(C_NULL); info = Vector{Int32}(undef, 1); y0 = zeros(Float64, n); d = Ref(desc(θ))
    GC.@preserve Xm y0 begin
        rc = ccall((:pmk_fit_batched, libpmk), Cint,
            (Ptr{Cvoid}, Ref{KernelDesc}, Float64, Cint, Int64, Ptr{Int64}, Ptr{Ptr{Float64}}, Ptr{Ptr{Float64}},
             Ref{Ptr{Cvoid}}, Ptr{Ptr{Float64}}, Ptr{Int32}),
            context(), d, σ², D, 1, Int64[n], [pointer(Xm)], [pointer(y0)], h, C_NULL, info)
    end
    check(rc, "setupGPquery")
    info[1] == 0 || throw(PosDefException(Int(info[1])))
    cc = Vector{Float64}(c)
    GC.@preserve cc check(ccall((:pmk_model_set_weights, libpmk), Cint, (Ptr{Cvoid}, Ptr{Ptr{Float64}}), h[], [pointer(cc)]),
                          "pmk_model_set_weights")
    model = Ref(h[])
    finalizer(m -> (ccall((:pmk_model_destroy, libpmk), Cvoid, (Ptr{Cvoid},), m[]); nothing), model)
    return xx -> evalqueryGP!(model, xx, θ)
end
function evalqueryGP!(model::Ref{Ptr{Cvoid}}, xq::Vector{T}, θ)::Tuple{T,T} where T
    Qm = kpack(θ, [xq]); μ = Ref(0.0); v = Ref(0.0)
    check(ccall((:pmk_model_queryinner_ex, libpmk), Cint,
        (Ptr{Cvoid}, Int64, Ref{KernelDesc}, Int64, Ptr{Float64}, Float64, Ref{Float64}, Ref{Float64}),
        model[], 0, Ref(desc(θ)), 1, Qm, -Inf, μ, v), "evalqueryGP!")
    return μ[], v[]
end

"""evalquery(x, c, X, θ) (src/RKHS/querying.jl:2-5)"""
function evalquery(x::Vector{T}, c::Vector{T}, X::Vector{Vector{T}}, θ)::T where T
    y = Vector{T}(undef, 1)
    query!(y, [x], RKHSProblemType(c, X, θ, zero(T)))
    return y[1]
end

end # module
