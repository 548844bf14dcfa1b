# PoleeHIP.jl -- thin ccall layer over libpolee_hip.so (include/polee_hip.h).
#
# This is the reference-side binding a Polee maintainer would add: it keeps the Julia
# function API of the hot path (names and argument order of src/ptt.jl, src/likelihood.jl,
# src/likelihood-approximation.jl, src/approx-sampler.jl) and routes it to the MI355X
# kernels, replacing PyCall + TensorFlow + hsb_ops.so.  NOT EXECUTED in the build container
# (no Julia there); the Python mirror polee_amd/core.py exercises the same C entry points, and
# julia/runtests.jl is the test-suite a box with Julia + an MI355X runs (it reads the reference's own
# HDF5 fixtures, test/dataset/mBr_M_6w_1.*.h5).
module PoleeHIP

const LIB = get(ENV, "POLEE_HIP_LIB", joinpath(@__DIR__, "..", "polee_amd", "csrc", "libpolee_hip.so"))

struct PoleeHIPError <: Exception
    status::Cint
    msg::String
end

function check(status::Cint, ctx::Ptr{Cvoid}=C_NULL)
    status == 0 && return
    msg = unsafe_string(ccall((:polee_last_error, LIB), Cstring, (Ptr{Cvoid},), ctx))
    # POLEE_ERR_NONFINITE (4) mirrors `@assert isfinite(...)` (likelihood-approximation.jl:559)
    status == 4 ? throw(AssertionError(msg)) : throw(PoleeHIPError(status, msg))
end

mutable struct Context
    h::Ptr{Cvoid}
    function Context(device::Integer=0)
        r = Ref{Ptr{Cvoid}}(C_NULL)
        check(ccall((:polee_ctx_create, LIB), Cint, (Cint, Ref{Ptr{Cvoid}}), device, r))
        c = new(r[])
        finalizer(c -> ccall((:polee_ctx_destroy, LIB), Cvoid, (Ptr{Cvoid},), c.h), c)
        return c
    end
end

# ---- PolyaTreeTransform (src/ptt.jl:6-27, 89-116) ------------------------------------
mutable struct PolyaTreeTransform
    h::Ptr{Cvoid}
    ctx::Context
    n::Int
    function PolyaTreeTransform(ctx::Context, parent_idxs::Vector{Int32}, output_idxs::Vector{Int32})
        @assert length(parent_idxs) == length(output_idxs)
        r = Ref{Ptr{Cvoid}}(C_NULL)
        GC.@preserve parent_idxs output_idxs check(
            ccall((:polee_ptt_create, LIB), Cint, (Ptr{Cvoid}, Ptr{Int32}, Ptr{Int32}, Int32, Ref{Ptr{Cvoid}}),
                  ctx.h, parent_idxs, output_idxs, length(parent_idxs), r), ctx.h)
        t = new(r[], ctx, div(length(parent_idxs) + 1, 2))
        finalizer(t -> ccall((:polee_ptt_destroy, LIB), Cvoid, (Ptr{Cvoid},), t.h), t)
        return t
    end
end

"transform!(t, ys, xs, Val(compute_ladj)) -- src/ptt.jl:125-160"
function transform!(t::PolyaTreeTransform, ys::Vector{Float64}, xs::Vector{Float32},
                    ::Val{compute_ladj}=Val(false)) where {compute_ladj}
    ladj = Ref{Float64}(0.0)
    GC.@preserve ys xs check(
        ccall((:polee_ptt_transform, LIB), Cint, (Ptr{Cvoid}, Ptr{Float64}, Int32, Ptr{Float32}, Ptr{Float64}),
              t.h, ys, 1, xs, compute_ladj ? ladj : C_NULL), t.ctx.h)
    return ladj[]
end

"transform_gradients!(t, ys, y_grad, x_grad) -- src/ptt.jl:167-209"
function transform_gradients!(t::PolyaTreeTransform, ys::Vector{Float64}, y_grad::AbstractVector,
                              x_grad::Vector{Float64}; with_ladj::Bool=true)
    tmp = Vector{Float64}(undef, t.n - 1)
    GC.@preserve ys x_grad tmp check(
        ccall((:polee_ptt_transform_gradients, LIB), Cint,
              (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}, Int32, Cint, Ptr{Float64}),
              t.h, ys, x_grad, 1, with_ladj, tmp), t.ctx.h)
    y_grad .= tmp   # the reference's y_grad is Float32 (likelihood-approximation.jl:466)
    return nothing
end
transform_gradients_no_ladj!(t, ys, y_grad, x_grad) = transform_gradients!(t, ys, y_grad, x_grad, with_ladj=false)

"inverse_transform!(t, xs, ys) -- src/ptt.jl:257-285"
function inverse_transform!(t::PolyaTreeTransform, xs::Vector{Float32}, ys::Vector{Float64})
    ladj = Ref{Float64}(0.0)
    GC.@preserve xs ys check(
        ccall((:polee_ptt_inverse_transform, LIB), Cint, (Ptr{Cvoid}, Ptr{Float32}, Int32, Ptr{Float64}, Ptr{Float64}),
              t.h, xs, 1, ys, ladj), t.ctx.h)
    return ladj[]
end

# ---- X + log_likelihood (src/likelihood.jl:2-56, src/sparse.jl) -----------------------
mutable struct DeviceSample
    h::Ptr{Cvoid}
    ctx::Context
    m::Int
    n::Int
    "X::SparseMatrixCSC{Float32,UInt32} exactly as RNASeqSample holds it (src/rnaseq_sample.jl:11)"
    function DeviceSample(ctx::Context, m, n, colptr::Vector{UInt32}, rowval::Vector{UInt32},
                          nzval::Vector{Float32}; ks::Union{Nothing,Vector{Int64}}=nothing)
        r = Ref{Ptr{Cvoid}}(C_NULL)
        GC.@preserve colptr rowval nzval ks check(
            ccall((:polee_loglik_create, LIB), Cint,
                  (Ptr{Cvoid}, Int64, Int64, Ptr{Cvoid}, Cint, Ptr{UInt32}, Ptr{Float32}, Ptr{Int64}, Ref{Ptr{Cvoid}}),
                  ctx.h, m, n, colptr, 4, rowval, nzval, ks === nothing ? C_NULL : ks, r), ctx.h)
        s = new(r[], ctx, m, n)
        finalizer(s -> ccall((:polee_loglik_destroy, LIB), Cvoid, (Ptr{Cvoid},), s.h), s)
        return s
    end
end

"log_likelihood(..., xs, x_grad, Val(gradonly)) -- src/likelihood.jl:36-56 (frag_probs scratch lives on the GPU)"
function log_likelihood(s::DeviceSample, xs::Vector{Float32}, x_grad::Vector{Float64},
                        ::Val{gradonly}) where {gradonly}
    lp = Ref{Float64}(0.0)
    GC.@preserve xs x_grad check(
        ccall((:polee_loglik_eval, LIB), Cint, (Ptr{Cvoid}, Ptr{Float32}, Int32, Ptr{Float64}, Ptr{Float64}),
              s.h, xs, 1, x_grad, gradonly ? C_NULL : lp), s.ctx.h)
    return lp[]
end

# ---- approximate_likelihood (src/likelihood-approximation.jl:395-624) -----------------
# Mirrors `struct polee_vi_opts`; obtain defaults with polee_vi_default_opts.
mutable struct ViOpts
    num_steps::Int32; num_mc_samples::Int32; use_efflen_jacobian::Int32; gradonly::Int32
    seed::UInt64; z0::Ptr{Float32}; y_eps::Float64
    adam_initial_learning_rate::Float64; adam_learning_rate_decay::Float64; adam_min_learning_rate::Float64
    adam_eps::Float64; adam_rv::Float64; adam_rm::Float64
    max_mu_step::Float64; max_omega_step::Float64; max_alpha_step::Float64
    profile::Int32; deterministic::Int32
    gene_of::Ptr{Int32}   # optional: gene index of every transcript (0-based, -1 = none known) = gene_noninformative
    ViOpts() = (o = new(); ccall((:polee_vi_default_opts, LIB), Cvoid, (Ref{ViOpts},), o); o)
end

"""
approximate_likelihood(::LogitSkewNormalPTTApprox, sample) replacement: returns the params Dict
("mu", "omega", "alpha") exactly as likelihood-approximation.jl:615-623 does.
"""
function approximate_likelihood(s::DeviceSample, t::PolyaTreeTransform, efflens::Vector{Float32};
                                use_efflen_jacobian::Bool=true, seed::Integer=123456789,
                                gene_transcripts::Union{Nothing,Dict{String,Vector{Int}}}=nothing,  # gene_noninformative
                                deterministic::Union{Nothing,Bool}=nothing)
    # (polee_vi_opts.deterministic: 0 = the library's rule, on exactly when the sample is shared by more than one rank; 1 on; -1 off)
    o = ViOpts(); o.use_efflen_jacobian = use_efflen_jacobian; o.seed = seed
    o.deterministic = deterministic === nothing ? 0 : (deterministic ? 1 : -1)
    # the reference's Dict{gene id -> transcript indexes} (likelihood-approximation.jl:475-487) as gene_of[n]
    gene_of = Int32[]
    if gene_transcripts !== nothing && !isempty(gene_transcripts)
        gene_of = fill(Int32(-1), s.n)
        for (gi, idxs) in enumerate(values(gene_transcripts)), i in idxs
            gene_of[i] = gi - 1
        end
        o.gene_of = pointer(gene_of)
    end
    mu = Vector{Float32}(undef, s.n - 1); omega = similar(mu); alpha = similar(mu)
    GC.@preserve efflens mu omega alpha gene_of check(
        ccall((:polee_vi_fit, LIB), Cint,
              (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float32}, Ref{ViOpts}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Cvoid}),
              s.h, t.h, efflens, o, mu, omega, alpha, C_NULL), s.ctx.h)
    return Dict{String,Vector}("mu" => mu, "omega" => omega, "alpha" => alpha)
end

"rand!(als, xs) -- src/approx-sampler.jl:37-44"
function rand_draws!(t::PolyaTreeTransform, mu::Vector{Float32}, sigma::Vector{Float32}, alpha::Vector{Float32},
                     xs::Matrix{Float32}; seed::Integer=rand(UInt64))   # xs is n x ndraws (column = one draw)
    GC.@preserve mu sigma alpha xs check(
        ccall((:polee_sampler_draw, LIB), Cint,
              (Ptr{Cvoid}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Int32, UInt64, Ptr{Float32}),
              t.h, mu, sigma, alpha, C_NULL, size(xs, 2), seed, xs), t.ctx.h)
    return xs
end

"x0 of load_samples_hdf5 -- src/estimate.jl:436-455: mean of N draws (y clamped, / efflens, renormalised)"
function initial_values(t::PolyaTreeTransform, mu::Vector{Float32}, sigma::Vector{Float32}, alpha::Vector{Float32},
                        efflens::Vector{Float32}, N::Integer=30; seed::Integer=rand(UInt64))
    x0 = Vector{Float32}(undef, length(mu) + 1)
    GC.@preserve mu sigma alpha efflens x0 check(
        ccall((:polee_sampler_initial_values, LIB), Cint,
              (Ptr{Cvoid}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Int32, UInt64, Ptr{Float32}),
              t.h, mu, sigma, alpha, efflens, C_NULL, N, seed, x0), t.ctx.h)
    return x0
end

"one sample of posterior_mean(loaded_samples, N) -- src/approx-sampler.jl:86-117"
function posterior_mean(t::PolyaTreeTransform, mu::Vector{Float32}, sigma::Vector{Float32}, alpha::Vector{Float32},
                        N::Integer=100; seed::Integer=rand(UInt64))
    pm = Vector{Float32}(undef, length(mu) + 1)
    GC.@preserve mu sigma alpha pm check(
        ccall((:polee_sampler_posterior_mean, LIB), Cint,
              (Ptr{Cvoid}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Int32, UInt64, Ptr{Float32}),
              t.h, mu, sigma, alpha, C_NULL, N, seed, pm), t.ctx.h)
    return pm
end

"one sample of Statistics.quantile(loaded_samples, transforms, qs, N) -- src/approx-sampler.jl:50-83; n x length(qs)"
function quantiles(t::PolyaTreeTransform, mu::Vector{Float32}, sigma::Vector{Float32}, alpha::Vector{Float32},
                   qs::Vector{Float64}=[0.01, 0.99], N::Integer=100; seed::Integer=rand(UInt64))
    out = Matrix{Float32}(undef, length(mu) + 1, length(qs))
    GC.@preserve mu sigma alpha qs out check(
        ccall((:polee_sampler_quantiles, LIB), Cint,
              (Ptr{Cvoid}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Int32, UInt64, Ptr{Float64}, Int32,
               Ptr{Float32}),
              t.h, mu, sigma, alpha, C_NULL, N, seed, qs, length(qs), out), t.ctx.h)
    return out
end

"effective_length_jacobian_adjustment!(efflens, xs, xls, x_grad) -- src/likelihood.jl:93-110"
function effective_length_jacobian_adjustment!(ctx::Context, efflens::Vector{Float32}, xs::Vector{Float32},
                                               xls::Vector{Float32}, x_grad::Vector{Float64})
    GC.@preserve efflens xs xls x_grad check(
        ccall((:polee_efflen_jacobian_adjustment, LIB), Cint,
              (Ptr{Cvoid}, Ptr{Float32}, Ptr{Float32}, Int32, Int64, Ptr{Float64}, Ptr{Float32}),
              ctx.h, efflens, xs, 1, length(xs), x_grad, xls), ctx.h)
    return 0.0
end

"gene_noninformative_prior!(efflens, xls, xl_grad, xs, x_grad, gene_transcripts) -- src/likelihood.jl:114-159"
function gene_noninformative_prior!(ctx::Context, efflens::Vector{Float32}, xls::Vector{Float32}, xs::Vector{Float32},
                                    x_grad::Vector{Float64}, gene_transcripts::Dict{String, Vector{Int}})
    gene_of = fill(Int32(-1), length(xs))
    for (gi, idxs) in enumerate(values(gene_transcripts)), i in idxs
        gene_of[i] = Int32(gi - 1)
    end
    GC.@preserve efflens xls xs x_grad gene_of check(
        ccall((:polee_gene_noninformative_prior, LIB), Cint,
              (Ptr{Cvoid}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Int32, Int64, Ptr{Int32}, Ptr{Float64}),
              ctx.h, efflens, xls, xs, 1, length(xs), gene_of, x_grad), ctx.h)
    return 0.0
end

# ---- one sample over several GPUs (one Julia process per GPU) -------------------------
"128-byte id for polee_comm_create; rank 0 creates it and the caller broadcasts it (MPI.jl, a file, ...)"
function comm_unique_id()
    id = Vector{UInt8}(undef, 128)
    GC.@preserve id check(ccall((:polee_comm_unique_id, LIB), Cint, (Ptr{UInt8},), id))
    return id
end

mutable struct Comm
    h::Ptr{Cvoid}
    ctx::Context
    function Comm(ctx::Context, nranks::Integer, rank::Integer, id::Vector{UInt8})
        out = Ref{Ptr{Cvoid}}(C_NULL)
        GC.@preserve id check(ccall((:polee_comm_create, LIB), Cint,
                                    (Ptr{Cvoid}, Int32, Int32, Ptr{UInt8}, Ref{Ptr{Cvoid}}),
                                    ctx.h, nranks, rank, id, out), ctx.h)
        c = new(out[], ctx)
        finalizer(x -> ccall((:polee_comm_destroy, LIB), Cvoid, (Ptr{Cvoid},), x.h), c)
        return c
    end
end

# ---- the VI loop as a handle (polee_vi_create / run / sync): step the fit, inspect it, shard it ----------------
mutable struct ViStats
    steps_done::Int32
    nonfinite_step::Int32
    loglik_kernel_ms_avg::Float64
    loglik_kernel_launches::Int64
    last_elbo::Float64
    last_lp_mean::Float64
    loglik_pass_ms_avg::Float64
    ViStats() = new(0, 0, 0.0, 0, 0.0, 0.0, 0.0)
end

"State of one fit of approximate_likelihood(::LogitSkewNormalPTTApprox, ...) (likelihood-approximation.jl:395-624)"
mutable struct LikelihoodApproximationFit
    h::Ptr{Cvoid}
    sample::DeviceSample
    t::PolyaTreeTransform
    function LikelihoodApproximationFit(s::DeviceSample, t::PolyaTreeTransform, efflens::Vector{Float32}, opts::ViOpts=ViOpts())
        out = Ref{Ptr{Cvoid}}(C_NULL)
        GC.@preserve efflens check(ccall((:polee_vi_create, LIB), Cint,
                                         (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float32}, Ref{ViOpts}, Ref{Ptr{Cvoid}}),
                                         s.h, t.h, efflens, opts, out), t.ctx.h)
        f = new(out[], s, t)
        finalizer(x -> ccall((:polee_vi_destroy, LIB), Cvoid, (Ptr{Cvoid},), x.h), f)
        return f
    end
end

"enqueue nsteps iterations (no host synchronisation)"
run!(f::LikelihoodApproximationFit, nsteps::Integer) =
    check(ccall((:polee_vi_run, LIB), Cint, (Ptr{Cvoid}, Int32), f.h, nsteps), f.t.ctx.h)
"wait for the stream; throws AssertionError on a non-finite gradient (likelihood-approximation.jl:559)"
sync!(f::LikelihoodApproximationFit) = check(ccall((:polee_vi_sync, LIB), Cint, (Ptr{Cvoid},), f.h), f.t.ctx.h)

function params(f::LikelihoodApproximationFit)
    n = f.t.n
    mu, omega, alpha = (Vector{Float32}(undef, n - 1) for _ in 1:3)
    GC.@preserve mu omega alpha check(ccall((:polee_vi_get_params, LIB), Cint,
                                            (Ptr{Cvoid}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}), f.h, mu, omega, alpha), f.t.ctx.h)
    return mu, omega, alpha
end

function set_params!(f::LikelihoodApproximationFit, mu::Vector{Float32}, omega::Vector{Float32}, alpha::Vector{Float32})
    GC.@preserve mu omega alpha check(ccall((:polee_vi_set_params, LIB), Cint,
                                            (Ptr{Cvoid}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}), f.h, mu, omega, alpha), f.t.ctx.h)
end

function stats(f::LikelihoodApproximationFit)
    st = ViStats()
    check(ccall((:polee_vi_get_stats, LIB), Cint, (Ptr{Cvoid}, Ref{ViStats}), f.h, st), f.t.ctx.h)
    return st
end

"per-step ELBO and mean log-likelihood (gradonly == 0 only)"
function trace(f::LikelihoodApproximationFit)
    k = Int(stats(f).steps_done)
    elbo, lp = Vector{Float64}(undef, k), Vector{Float64}(undef, k)
    GC.@preserve elbo lp check(ccall((:polee_vi_get_trace, LIB), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}), f.h, elbo, lp), f.t.ctx.h)
    return elbo, lp
end

"row-sharded fit: this handle's sample holds one rank's block of fragments (SURVEY 8(e)(1))"
set_comm!(f::LikelihoodApproximationFit, c) =
    check(ccall((:polee_vi_set_comm, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}), f.h, c === nothing ? C_NULL : c.h), f.t.ctx.h)

# ---- tree construction: hclust + order_nodes (src/hclust.jl:193-319, 361-389) -----------------------------------
"X in CSC, 1-based (colptr UInt32 or UInt64), as in the likelihood-matrix HDF5 -> (node_parent_idxs, node_js)"
function hclust(m::Integer, n::Integer, colptr::Union{Vector{UInt32},Vector{UInt64}}, rowval::Vector{UInt32};
                parallel::Bool=false, device::Union{Nothing,Context}=nothing)
    parents, js = Vector{Int32}(undef, 2n - 1), Vector{Int32}(undef, 2n - 1)
    if device !== nothing   # the rounds variant built on the GPU: the same arrays as parallel = true
        GC.@preserve colptr rowval parents js check(
            ccall((:polee_hclust_parallel_device, LIB), Cint, (Ptr{Cvoid}, Int64, Int64, Ptr{Cvoid}, Cint, Ptr{UInt32}, Ptr{Int32}, Ptr{Int32}),
                  device.h, m, n, colptr, sizeof(eltype(colptr)), rowval, parents, js), device.h)
    elseif parallel   # rounds of mutually-best merges on all host threads: a variant, not hclust.jl's tree node for node
        GC.@preserve colptr rowval parents js check(
            ccall((:polee_hclust_parallel, LIB), Cint, (Int64, Int64, Ptr{Cvoid}, Cint, Ptr{UInt32}, Ptr{Int32}, Ptr{Int32}),
                  m, n, colptr, sizeof(eltype(colptr)), rowval, parents, js))
    else
        GC.@preserve colptr rowval parents js check(
            ccall((:polee_hclust, LIB), Cint, (Int64, Int64, Ptr{Cvoid}, Cint, Ptr{UInt32}, Ptr{Int32}, Ptr{Int32}),
                  m, n, colptr, sizeof(eltype(colptr)), rowval, parents, js))
    end
    return parents, js
end

# ---- tree from transcript sequences: polee fit-tree (src/main.jl:638-660, src/kmersketch.jl, src/kmercluster.jl) ----
"(offsets, bases) of sequences given as strings or byte vectors: the layout polee_kmer_sketch takes"
function concat_sequences(seqs)
    offsets = Vector{Int64}(undef, length(seqs) + 1)
    offsets[1] = 0
    for (i, s) in enumerate(seqs)
        offsets[i + 1] = offsets[i] + ncodeunits(String(s))
    end
    bases = Vector{UInt8}(undef, max(offsets[end], 1))
    for (i, s) in enumerate(seqs)
        copyto!(bases, offsets[i] + 1, codeunits(String(s)), 1, offsets[i + 1] - offsets[i])
    end
    return offsets, bases
end

"MinHash sketches of the canonical 32-mers, UInt64 [200, n] (column t = transcript t); ctx = nothing: on the host threads"
function kmer_sketches(seqs; ctx::Union{Nothing,Context}=nothing)
    offsets, bases = concat_sequences(seqs)
    n = length(seqs)
    sk = zeros(UInt64, 200, n)
    if ctx === nothing
        GC.@preserve offsets bases sk check(
            ccall((:polee_kmer_sketch_host, LIB), Cint, (Int64, Ptr{Int64}, Ptr{UInt8}, Ptr{UInt64}), n, offsets, bases, sk))
    else
        GC.@preserve offsets bases sk check(
            ccall((:polee_kmer_sketch, LIB), Cint, (Ptr{Cvoid}, Int64, Ptr{Int64}, Ptr{UInt8}, Ptr{UInt64}), ctx.h, n, offsets, bases, sk), ctx.h)
    end
    return sk
end

"sketches UInt64 [200, n] -> (node_parent_idxs, node_js); ctx = nothing: host only, else the candidate edges come from the GPU"
function kmer_tree(sk::Matrix{UInt64}; ctx::Union{Nothing,Context}=nothing)
    n = size(sk, 2)
    parents, js = Vector{Int32}(undef, 2n - 1), Vector{Int32}(undef, 2n - 1)
    if ctx === nothing
        GC.@preserve sk parents js check(
            ccall((:polee_kmer_tree_host, LIB), Cint, (Int64, Ptr{UInt64}, Ptr{Int32}, Ptr{Int32}), n, sk, parents, js))
    else
        GC.@preserve sk parents js check(
            ccall((:polee_kmer_tree, LIB), Cint, (Ptr{Cvoid}, Int64, Ptr{UInt64}, Ptr{Int32}, Ptr{Int32}), ctx.h, n, sk, parents, js), ctx.h)
    end
    return parents, js
end

"""
sketches UInt64 [200, n] -> (node_parent_idxs, node_js, stats) with the merges made in rounds of mutually-best pairs (DESIGN.md 3.12):
another tree than kmer_tree's, the same from the host threads (ctx = nothing) and from the GPU.  stats = (rounds, merges, nodes
left for the Huffman phase, pairs re-evaluated).
"""
function kmer_tree_rounds(sk::Matrix{UInt64}; ctx::Union{Nothing,Context}=nothing)
    n = size(sk, 2)
    parents, js, stats = Vector{Int32}(undef, 2n - 1), Vector{Int32}(undef, 2n - 1), zeros(Int64, 4)
    if ctx === nothing
        GC.@preserve sk parents js stats check(
            ccall((:polee_kmer_tree_rounds_host, LIB), Cint, (Int64, Ptr{UInt64}, Ptr{Int32}, Ptr{Int32}, Ptr{Int64}), n, sk, parents, js, stats))
    else
        GC.@preserve sk parents js stats check(
            ccall((:polee_kmer_tree_rounds, LIB), Cint, (Ptr{Cvoid}, Int64, Ptr{UInt64}, Ptr{Int32}, Ptr{Int32}, Ptr{Int64}),
                  ctx.h, n, sk, parents, js, stats), ctx.h)
    end
    return parents, js, stats
end

"build_polya_tree_transformation with the merges in rounds, wholly on the GPU (polee_fit_tree_rounds)"
function build_polya_tree_transformation_rounds(ctx::Context, seqs)
    offsets, bases = concat_sequences(seqs)
    n = length(seqs)
    parents, js, stats = Vector{Int32}(undef, 2n - 1), Vector{Int32}(undef, 2n - 1), zeros(Int64, 4)
    GC.@preserve offsets bases parents js stats check(
        ccall((:polee_fit_tree_rounds, LIB), Cint, (Ptr{Cvoid}, Int64, Ptr{Int64}, Ptr{UInt8}, Ptr{Int32}, Ptr{Int32}, Ptr{Int64}),
              ctx.h, n, offsets, bases, parents, js, stats), ctx.h)
    return parents, js, stats
end

"build_polya_tree_transformation (kmercluster.jl:96-262) on the GPU: the sketches stay on the device between the two steps"
function build_polya_tree_transformation(ctx::Context, seqs)
    offsets, bases = concat_sequences(seqs)
    n = length(seqs)
    parents, js = Vector{Int32}(undef, 2n - 1), Vector{Int32}(undef, 2n - 1)
    GC.@preserve offsets bases parents js check(
        ccall((:polee_fit_tree, LIB), Cint, (Ptr{Cvoid}, Int64, Ptr{Int64}, Ptr{UInt8}, Ptr{Int32}, Ptr{Int32}),
              ctx.h, n, offsets, bases, parents, js), ctx.h)
    return parents, js
end

"release the scratch blocks the host-side builders keep between samples"
host_cache_trim() = ccall((:polee_host_cache_trim, LIB), Cvoid, ())

# ---- density of the fitted approximations: replaces create_tensorflow_variables! (src/estimate.jl:502-556) +
#      RNASeqApproxLikelihoodDist (src/polee_approx_likelihood.py:367-450) -------------------------------------------
"""
    ApproxLikelihood(ctx, vars)

`vars` is `LoadedSamples.variables` (estimate.jl:502-556): "efflen" [S,n], "la_mu" / "la_sigma" / "la_alpha" [S,n-1],
"left_index" / "right_index" / "leaf_index" [S,N] (or [1,N] for one shared tree), as ROW-MAJOR C arrays -- i.e. pass
`permutedims` of Julia's column-major matrices, or vectors already laid out sample by sample.
"""
mutable struct ApproxLikelihood
    h::Ptr{Cvoid}
    ctx::Context
    S::Int
    n::Int
    function ApproxLikelihood(ctx::Context, S::Integer, n::Integer, efflen::Vector{Float32}, la_mu::Vector{Float32},
                              la_sigma::Vector{Float32}, la_alpha::Vector{Float32}, left_index::Vector{Int32},
                              right_index::Vector{Int32}, leaf_index::Vector{Int32}; shared_tree::Bool=false)
        out = Ref{Ptr{Cvoid}}(C_NULL)
        GC.@preserve efflen la_mu la_sigma la_alpha left_index right_index leaf_index check(
            ccall((:polee_approx_create, LIB), Cint,
                  (Ptr{Cvoid}, Int32, Int32, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Int32}, Ptr{Int32},
                   Ptr{Int32}, Cint, Ref{Ptr{Cvoid}}),
                  ctx.h, S, n, efflen, la_mu, la_sigma, la_alpha, left_index, right_index, leaf_index, shared_tree, out), ctx.h)
        a = new(out[], ctx, S, n)
        finalizer(x -> ccall((:polee_approx_destroy, LIB), Cvoid, (Ptr{Cvoid},), x.h), a)
        return a
    end
end

"log_prob(ap, x; grad) -- x Float32 [S*n] (sample by sample) unnormalised log expression -> lp [S] (, d lp / d x)"
function log_prob(ap::ApproxLikelihood, x::Vector{Float32}; grad::Bool=false)
    lp = Vector{Float32}(undef, ap.S)
    g = grad ? Vector{Float32}(undef, ap.S * ap.n) : Float32[]
    GC.@preserve x lp g check(ccall((:polee_approx_logprob, LIB), Cint, (Ptr{Cvoid}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}),
                                    ap.h, x, lp, grad ? pointer(g) : C_NULL), ap.ctx.h)
    return grad ? (lp, g) : lp
end

"rnaseq_approx_likelihood_sampler (polee_approx_likelihood.py:35-59): one draw per sample -> x Float32 [S*n]"
function sample(ap::ApproxLikelihood; seed::Integer=0, z0::Union{Nothing,Vector{Float32}}=nothing)
    x = Vector{Float32}(undef, ap.S * ap.n)
    GC.@preserve x z0 check(ccall((:polee_approx_sample, LIB), Cint, (Ptr{Cvoid}, Ptr{Float32}, UInt64, Ptr{Float32}),
                                  ap.h, z0 === nothing ? C_NULL : pointer(z0), seed, x), ap.ctx.h)
    return x
end

"RNASeqGeneApproxLikelihoodDist (polee_gene_expression.py:14-90); gene_of: 0-based gene of every transcript"
function gene_log_prob(ap::ApproxLikelihood, x_gene::Vector{Float32}, x_isoform::Vector{Float32}, gene_of::Vector{Int32},
                       num_genes::Integer; grad::Bool=false)
    lp = Vector{Float32}(undef, ap.S)
    gg = grad ? Vector{Float32}(undef, ap.S * num_genes) : Float32[]
    gi = grad ? Vector{Float32}(undef, ap.S * ap.n) : Float32[]
    GC.@preserve x_gene x_isoform gene_of lp gg gi check(
        ccall((:polee_approx_gene_logprob, LIB), Cint,
              (Ptr{Cvoid}, Ptr{Float32}, Ptr{Float32}, Ptr{Int32}, Int32, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}),
              ap.h, x_gene, x_isoform, gene_of, num_genes, lp, grad ? pointer(gg) : C_NULL, grad ? pointer(gi) : C_NULL), ap.ctx.h)
    return grad ? (lp, gg, gi) : lp
end

"approximate_feature_likelihood (polee_gene_expression.py:191-222): (loc, scale) Float32 [S*F]; pairs are 1-based"
function feature_moments(ap::ApproxLikelihood, feature_idxs::Vector{Int32}, transcript_idxs::Vector{Int32}, F::Integer;
                         num_mean_draws::Integer=1000, num_var_draws::Integer=1000, seed::Integer=0)
    loc, scale = Vector{Float32}(undef, ap.S * F), Vector{Float32}(undef, ap.S * F)
    GC.@preserve feature_idxs transcript_idxs loc scale check(
        ccall((:polee_approx_feature_moments, LIB), Cint,
              (Ptr{Cvoid}, Ptr{Int32}, Ptr{Int32}, Int64, Int32, Int32, Int32, UInt64, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}),
              ap.h, feature_idxs, transcript_idxs, length(feature_idxs), F, num_mean_draws, num_var_draws, seed, C_NULL, loc, scale),
        ap.ctx.h)
    return loc, scale
end

# ---- regression model: replaces the python-object protocol Regression(...).fit(niter)
#      (src/regression.jl:319-327, models/polee_regression.py:18-340) ------------------------------------------------
mutable struct Regression
    h::Ptr{Cvoid}
    ctx::Context
    S::Int
    F::Int
    n::Int
    """design Float32 [S*F], x_init Float32 [S*n] (row-major); hinges = nothing: choose_knots as
    RNASeqTranscriptLinearRegression does (models/polee_regression.py:436-440)"""
    function Regression(ctx::Context, ap::Union{Nothing,ApproxLikelihood}, S::Integer, F::Integer, n::Integer,
                        design::Vector{Float32}, x_init::Vector{Float32}, sample_scales::Vector{Float32};
                        x_init_mean::Union{Nothing,Vector{Float32}}=nothing, hinges::Union{Nothing,Vector{Float32}}=nothing,
                        degree::Integer=15, bandwidth::Real=1.0, x_bias_loc0::Real=log(1 / n), x_bias_scale0::Real=12.0,
                        use_distortion::Bool=true, scale_penalty::Real=1.0, use_point_estimates::Bool=false)
        out = Ref{Ptr{Cvoid}}(C_NULL)
        GC.@preserve design x_init sample_scales x_init_mean hinges check(
            ccall((:polee_regression_create, LIB), Cint,
                  (Ptr{Cvoid}, Ptr{Cvoid}, Int32, Int32, Int32, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32},
                   Int32, Cfloat, Cfloat, Cfloat, Cint, Cfloat, Cint, Ref{Ptr{Cvoid}}),
                  ctx.h, ap === nothing ? C_NULL : ap.h, S, F, n, design, x_init,
                  x_init_mean === nothing ? C_NULL : pointer(x_init_mean), sample_scales,
                  hinges === nothing ? C_NULL : pointer(hinges), degree, bandwidth, x_bias_loc0, x_bias_scale0, use_distortion,
                  scale_penalty, use_point_estimates, out), ctx.h)
        r = new(out[], ctx, S, F, n)
        finalizer(x -> ccall((:polee_regression_destroy, LIB), Cvoid, (Ptr{Cvoid},), x.h), r)
        return r
    end
end

num_params(r::Regression) = Int(ccall((:polee_regression_num_params, LIB), Int64, (Ptr{Cvoid},), r.h))

"fit(niter) (models/polee_regression.py:303-340); returns the loss trace"
function fit!(r::Regression, niter::Integer; seed::Integer=0)
    losses = Vector{Float32}(undef, niter)
    GC.@preserve losses check(ccall((:polee_regression_fit, LIB), Cint, (Ptr{Cvoid}, Int32, UInt64, Ptr{Float32}, Ptr{Float32}),
                                    r.h, niter, seed, C_NULL, losses), r.ctx.h)
    return losses
end

"the flat parameter vector (order documented in include/polee_hip.h)"
function flat_params(r::Regression)
    p = Vector{Float32}(undef, num_params(r))
    GC.@preserve p check(ccall((:polee_regression_get_params, LIB), Cint, (Ptr{Cvoid}, Ptr{Float32}), r.h, p), r.ctx.h)
    return p
end

"""
(qx_loc[S,n], qw_loc[F,n], qw_scale[F,n], qx_bias[n], qx_scale[n]) as `Regression(...).fit(niter)` returns them
(src/regression.jl:319-327): slices of the flat vector, softplus applied where the reference applies it.
"""
function fit_results(r::Regression; degree::Integer=15)
    p = flat_params(r)
    S, F, n = r.S, r.F, r.n
    softplus(x) = log1p(exp(x))
    o = 4 + F * degree + 2 * degree                     # scalars, distortion and mean-variance coefficients
    blk(k) = reshape(p[o + k * F * n + 1:o + (k + 1) * F * n], n, F)'   # k-th [F][n] array (row-major) as an F x n matrix
    qw_loc, qw_scale = blk(8), softplus.(blk(9))
    o += 10 * F * n
    qx_bias = p[o + 1:o + n]
    qx_scale = softplus.(p[o + 2n + 1:o + 3n])
    o += 4n
    qx_loc = reshape(p[o + 1:o + S * n], n, S)'
    return qx_loc, qw_loc, qw_scale, qx_bias, qx_scale
end

"samples sharded over ranks: one all-reduce of (F+2) n statistics per step (SURVEY 8(e)(2))"
set_comm!(r::Regression, c) =
    check(ccall((:polee_regression_set_comm, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}), r.h, c === nothing ? C_NULL : c.h), r.ctx.h)

"""
gene-level likelihood on a model created over the genes (ap = nothing): RNASeqGeneLinearRegression
(models/polee_regression.py:533-600), or with `F_isoform` (S x Fi) RNASeqGeneIsoformLinearRegression (:656-877).
`gene_of`: 1-based gene of every transcript; `x_isoform_init`: S x nt.
"""
function set_gene_likelihood!(r::Regression, ap::ApproxLikelihood, gene_of::AbstractVector{<:Integer},
                              x_isoform_init::AbstractMatrix; F_isoform::Union{Nothing,AbstractMatrix}=nothing)
    g = Int32.(gene_of .- 1)
    xi = Matrix{Float32}(x_isoform_init')            # row-major [S][nt]
    if F_isoform === nothing
        GC.@preserve g xi check(ccall((:polee_regression_set_gene_likelihood, LIB), Cint,
            (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Int32}, Ptr{Float32}), r.h, ap.h, g, xi), r.ctx.h)
    else
        Fi = Matrix{Float32}(F_isoform')             # row-major [S][Fi]
        GC.@preserve g xi Fi check(ccall((:polee_regression_set_gene_isoform_likelihood, LIB), Cint,
            (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Int32}, Ptr{Float32}, Ptr{Float32}, Int32),
            r.h, ap.h, g, xi, Fi, Int32(size(F_isoform, 2))), r.ctx.h)
    end
    return r
end

"""
RNASeqJointLinearRegression (models/polee_regression.py:879-1283) on a model created over the genes (ap = nothing, no
distortion, scale penalty 5e-4): gene block with a one-level horseshoe prior and kernel-regression weights of the sampled
bias, plus a regression over `num_splice_features` splice features that reaches the transcripts through the 0/1 matrix given
by the 1-based pairs (`feature_is`, `feature_js`) -- the arguments of models/joint-regression.jl.
"""
function set_joint_likelihood!(r::Regression, ap::ApproxLikelihood, gene_of::AbstractVector{<:Integer},
                               x_isoform_init::AbstractMatrix, num_splice_features::Integer,
                               feature_is::AbstractVector{<:Integer}, feature_js::AbstractVector{<:Integer})
    length(feature_is) == length(feature_js) || throw(ArgumentError("feature_is and feature_js must pair up"))
    g = Int32.(gene_of .- 1)
    xi = Matrix{Float32}(x_isoform_init')            # row-major [S][nt]
    pt = Int32.(feature_is .- 1)
    pf = Int32.(feature_js .- 1)
    GC.@preserve g xi pt pf check(ccall((:polee_regression_set_joint_likelihood, LIB), Cint,
        (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Int32}, Ptr{Float32}, Int32, Ptr{Int32}, Ptr{Int32}, Int64),
        r.h, ap.h, g, xi, Int32(num_splice_features), pt, pf, Int64(length(pt))), r.ctx.h)
    return r
end

"Adam step size of fit (2e-3 as created; the joint model sets 1e-3, models/polee_regression.py:1222)"
set_learning_rate!(r::Regression, lr::Real) =
    check(ccall((:polee_regression_set_learning_rate, LIB), Cint, (Ptr{Cvoid}, Cfloat), r.h, Float32(lr)), r.ctx.h)

"the isoform block of a gene-level / gene-isoform model as a flat vector (order: include/polee_hip.h)"
function isoform_params(r::Regression)
    n = Int(ccall((:polee_regression_num_isoform_params, LIB), Int64, (Ptr{Cvoid},), r.h))
    p = Vector{Float32}(undef, n)
    GC.@preserve p check(ccall((:polee_regression_get_isoform_params, LIB), Cint, (Ptr{Cvoid}, Ptr{Float32}), r.h, p), r.ctx.h)
    return p
end

# ---- host-staged communicator: the all-reduce is the caller's (e.g. MPI.Allreduce!) ----------------------------------
mutable struct HostComm
    h::Ptr{Cvoid}
    ctx::Context
    allreduce::Function     # (buf::Vector{Float32} or Vector{Float64}) -> sums it over the ranks in place
    cfun::Base.CFunction
    function HostComm(ctx::Context, nranks::Integer, rank::Integer, allreduce::Function)
        cb = function (user::Ptr{Cvoid}, buf::Ptr{Cvoid}, count::Int64, is_f64::Cint)::Cint
            try
                a = is_f64 != 0 ? unsafe_wrap(Array, Ptr{Float64}(buf), count) : unsafe_wrap(Array, Ptr{Float32}(buf), count)
                allreduce(a)
                return Cint(0)
            catch
                return Cint(1)
            end
        end
        cfun = @cfunction($cb, Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Int64, Cint))
        out = Ref{Ptr{Cvoid}}(C_NULL)
        check(ccall((:polee_comm_create_host, LIB), Cint, (Ptr{Cvoid}, Int32, Int32, Ptr{Cvoid}, Ptr{Cvoid}, Ref{Ptr{Cvoid}}),
                    ctx.h, nranks, rank, cfun, C_NULL, out), ctx.h)
        c = new(out[], ctx, allreduce, cfun)
        finalizer(x -> ccall((:polee_comm_destroy, LIB), Cvoid, (Ptr{Cvoid},), x.h), c)
        return c
    end
end


# =====================================================================================================================
# Round 4: the rest of the C ABI (every export of libpolee_hip.so now has a wrapper; julia/runtests.jl exercises them
# against the golden fixtures).  Reference call sites in the docstrings.
# =====================================================================================================================

version() = unsafe_string(ccall((:polee_version, LIB), Cstring, ()))
synchronize(ctx::Context) = check(ccall((:polee_ctx_synchronize, LIB), Cint, (Ptr{Cvoid},), ctx.h), ctx.h)
"the context's hipStream_t (for callers that enqueue their own HIP work behind the library's)"
stream(ctx::Context) = ccall((:polee_ctx_stream, LIB), Ptr{Cvoid}, (Ptr{Cvoid},), ctx.h)
"(free, total) bytes of the context's GPU"
function mem_info(ctx::Context)
    f, t = Ref{Int64}(0), Ref{Int64}(0)
    check(ccall((:polee_ctx_mem_info, LIB), Cint, (Ptr{Cvoid}, Ref{Int64}, Ref{Int64}), ctx.h, f, t), ctx.h)
    return f[], t[]
end
"HIP-event stopwatch on the context's stream"
timer_start(ctx::Context) = check(ccall((:polee_ctx_timer_start, LIB), Cint, (Ptr{Cvoid},), ctx.h), ctx.h)
function timer_stop(ctx::Context)
    ms = Ref{Float64}(0.0)
    check(ccall((:polee_ctx_timer_stop, LIB), Cint, (Ptr{Cvoid}, Ref{Float64}), ctx.h, ms), ctx.h)
    return ms[]
end
"cap (MB) of the host builders' scratch-block cache; cap_mb < 0 only queries.  Returns the cap in force."
host_cache_configure(cap_mb::Integer=-1) = ccall((:polee_host_cache_configure, LIB), Int64, (Int64,), cap_mb)
host_cache_bytes() = ccall((:polee_host_cache_bytes, LIB), Int64, ())
"device bytes the library keeps for its next allocations (host_cache_trim() frees them too)"
device_cache_bytes() = ccall((:polee_device_cache_bytes, LIB), Int64, ())

# ---- trees from the TF-side index arrays; the three TF custom ops (src/tensorflow_ext/hsb_ops.cpp) -------------------
"make_inverse_ptt_params(t) -- src/estimate.jl:461-500: (left_index, right_index, leaf_index), 0-based, -1 = none"
function make_inverse_ptt_params(parent_idxs::Vector{Int32}, output_idxs::Vector{Int32})
    N = length(parent_idxs)
    l, r, f = (Vector{Int32}(undef, N) for _ in 1:3)
    GC.@preserve parent_idxs output_idxs l r f check(
        ccall((:polee_make_inverse_ptt_params, LIB), Cint, (Ptr{Int32}, Ptr{Int32}, Int32, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}),
              parent_idxs, output_idxs, N, l, r, f))
    return l, r, f
end

"a tree handle from the index arrays the TF ops take (hsb_ops.cpp:17-60)"
function tree_from_index(ctx::Context, left_index::Vector{Int32}, right_index::Vector{Int32}, leaf_index::Vector{Int32})
    out = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve left_index right_index leaf_index check(
        ccall((:polee_ptt_create_from_index, LIB), Cint, (Ptr{Cvoid}, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}, Int32, Ref{Ptr{Cvoid}}),
              ctx.h, left_index, right_index, leaf_index, length(left_index), out), ctx.h)
    t = PolyaTreeTransformHandle(out[], ctx)
    return t
end
"a bare tree handle (trees created from index arrays have no parent / js arrays on the Julia side)"
mutable struct PolyaTreeTransformHandle
    h::Ptr{Cvoid}
    ctx::Context
    function PolyaTreeTransformHandle(h::Ptr{Cvoid}, ctx::Context)
        t = new(h, ctx)
        finalizer(x -> ccall((:polee_ptt_destroy, LIB), Cvoid, (Ptr{Cvoid},), x.h), t)
        return t
    end
end
const AnyTree = Union{PolyaTreeTransform,PolyaTreeTransformHandle}
num_leaves(t::AnyTree) = Int(ccall((:polee_ptt_n, LIB), Int32, (Ptr{Cvoid},), t.h))

"TF op HSB (hsb_ops.cpp:62-121): y_logit Float32 [B*(n-1)] row-major -> x Float32 [B*n]"
function hsb(t::AnyTree, y_logit::Vector{Float32}, B::Integer=1)
    x = Vector{Float32}(undef, B * num_leaves(t))
    GC.@preserve y_logit x check(ccall((:polee_hsb, LIB), Cint, (Ptr{Cvoid}, Ptr{Float32}, Int32, Ptr{Float32}), t.h, y_logit, B, x), t.ctx.h)
    return x
end
"TF op InvHSB (hsb_ops.cpp:123-250): x [B*n] -> (y Float64 [B*(n-1)], ladj Float32 [B])"
function inv_hsb(t::AnyTree, x::Vector{Float32}, B::Integer=1)
    y, ladj = Vector{Float64}(undef, B * (num_leaves(t) - 1)), Vector{Float32}(undef, B)
    GC.@preserve x y ladj check(ccall((:polee_inv_hsb, LIB), Cint, (Ptr{Cvoid}, Ptr{Float32}, Int32, Ptr{Float64}, Ptr{Float32}),
                                      t.h, x, B, y, ladj), t.ctx.h)
    return y, ladj
end
"TF op InvHSBGrad (hsb_ops.cpp:252-402): -> backprops Float32 [B*n]"
function inv_hsb_grad(t::AnyTree, y_grad::Vector{Float64}, ladj_grad::Vector{Float32}, y::Vector{Float64}, B::Integer=1)
    bp = Vector{Float32}(undef, B * num_leaves(t))
    GC.@preserve y_grad ladj_grad y bp check(
        ccall((:polee_inv_hsb_grad, LIB), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float32}, Ptr{Float64}, Int32, Ptr{Float32}),
              t.h, y_grad, ladj_grad, y, B, bp), t.ctx.h)
    return bp
end

# ---- the reparameterisations as standalone calls (src/logitnormal.jl, src/sinh_arcsinh.jl, src/kumaraswamy.jl) -------
"logit_normal_transform!(mu, sigma, zs, ys, Val(compute_ladj)) -- src/logitnormal.jl:8-20"
function logit_normal_transform!(ctx::Context, mu::Vector{Float32}, sigma::Vector{Float32}, zs::Vector{Float32},
                                 ys::Vector{Float64}, ::Val{compute_ladj}=Val(false)) where {compute_ladj}
    ladj = Ref{Float64}(0.0)
    GC.@preserve mu sigma zs ys check(
        ccall((:polee_logit_normal_transform, LIB), Cint, (Ptr{Cvoid}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Int64, Ptr{Float64}, Ptr{Float64}),
              ctx.h, mu, sigma, zs, length(zs), ys, compute_ladj ? ladj : C_NULL), ctx.h)
    return ladj[]
end
"logit_normal_transform_gradients!(zs, ys, mu, sigma, y_grad, z_grad, mu_grad, sigma_grad) -- src/logitnormal.jl:38-55 (accumulates)"
function logit_normal_transform_gradients!(ctx::Context, zs::Vector{Float32}, ys::Vector{Float64}, sigma::Vector{Float32},
                                           y_grad::Vector{Float32}, z_grad::Union{Nothing,Vector{Float32}},
                                           mu_grad::Vector{Float32}, sigma_grad::Vector{Float32})
    GC.@preserve zs ys sigma y_grad z_grad mu_grad sigma_grad check(
        ccall((:polee_logit_normal_transform_gradients, LIB), Cint,
              (Ptr{Cvoid}, Ptr{Float32}, Ptr{Float64}, Ptr{Float32}, Ptr{Float32}, Int64, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}),
              ctx.h, zs, ys, sigma, y_grad, length(zs), z_grad === nothing ? C_NULL : pointer(z_grad), mu_grad, sigma_grad), ctx.h)
    return nothing
end
"sinh_asinh_transform!(alpha, zs0, zs, Val(compute_ladj)) -- src/sinh_arcsinh.jl:10-23"
function sinh_asinh_transform!(ctx::Context, alpha::Vector{Float32}, zs0::Vector{Float32}, zs::Vector{Float32},
                               ::Val{compute_ladj}=Val(false)) where {compute_ladj}
    ladj = Ref{Float64}(0.0)
    GC.@preserve alpha zs0 zs check(
        ccall((:polee_sinh_asinh_transform, LIB), Cint, (Ptr{Cvoid}, Ptr{Float32}, Ptr{Float32}, Int64, Ptr{Float32}, Ptr{Float64}),
              ctx.h, alpha, zs0, length(zs0), zs, compute_ladj ? ladj : C_NULL), ctx.h)
    return ladj[]
end
"sinh_asinh_transform_gradients!(zs0, alpha, z_grad, alpha_grad) -- src/sinh_arcsinh.jl:29-38 (accumulates)"
function sinh_asinh_transform_gradients!(ctx::Context, zs0::Vector{Float32}, alpha::Vector{Float32}, z_grad::Vector{Float32},
                                         alpha_grad::Vector{Float32})
    GC.@preserve zs0 alpha z_grad alpha_grad check(
        ccall((:polee_sinh_asinh_transform_gradients, LIB), Cint, (Ptr{Cvoid}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Int64, Ptr{Float32}),
              ctx.h, zs0, alpha, z_grad, length(zs0), alpha_grad), ctx.h)
    return nothing
end
"kumaraswamy_transform!(as, bs, zs, ys, Val(compute_ladj)) -- src/kumaraswamy.jl:9-36"
function kumaraswamy_transform!(ctx::Context, as::Vector{Float32}, bs::Vector{Float32}, zs::Vector{Float32},
                                ys::Vector{Float64}, ::Val{compute_ladj}=Val(false)) where {compute_ladj}
    ladj = Ref{Float64}(0.0)
    GC.@preserve as bs zs ys check(
        ccall((:polee_kumaraswamy_transform, LIB), Cint, (Ptr{Cvoid}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Int64, Ptr{Float64}, Ptr{Float64}),
              ctx.h, as, bs, zs, length(zs), ys, compute_ladj ? ladj : C_NULL), ctx.h)
    return ladj[]
end
"kumaraswamy_transform_gradients!(zs, as, bs, y_grad, a_grad, b_grad) -- src/kumaraswamy.jl:39-71 (accumulates)"
function kumaraswamy_transform_gradients!(ctx::Context, zs::Vector{Float32}, as::Vector{Float32}, bs::Vector{Float32},
                                          y_grad::Vector{Float32}, a_grad::Vector{Float32}, b_grad::Vector{Float32})
    GC.@preserve zs as bs y_grad a_grad b_grad check(
        ccall((:polee_kumaraswamy_transform_gradients, LIB), Cint,
              (Ptr{Cvoid}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Int64, Ptr{Float32}, Ptr{Float32}),
              ctx.h, zs, as, bs, y_grad, length(zs), a_grad, b_grad), ctx.h)
    return nothing
end

# ---- the sample from the rows of X; layout information; deterministic mode ------------------------------------------
"X given by rows (Xt = SparseMatrixCSC(transpose(X)), likelihood-approximation.jl:407): tcolptr UInt64 [m+1] 1-based"
function DeviceSampleFromXt(ctx::Context, m, n, tcolptr::Vector{UInt64}, trowval::Vector{UInt32}, tnzval::Vector{Float32};
                            ks::Union{Nothing,Vector{Int64}}=nothing)
    r = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve tcolptr trowval tnzval ks check(
        ccall((:polee_loglik_create_from_xt, LIB), Cint,
              (Ptr{Cvoid}, Int64, Int64, Ptr{UInt64}, Ptr{UInt32}, Ptr{Float32}, Ptr{Int64}, Ref{Ptr{Cvoid}}),
              ctx.h, m, n, tcolptr, trowval, tnzval, ks === nothing ? C_NULL : pointer(ks), r), ctx.h)
    return wrap_sample(r[], ctx, m, n)
end
"true: the device layout of this sample was built by the device builder (csrc/psell_device.hip); false: by the host builder"
built_on_device(s) = ccall((:polee_loglik_built_on_device, LIB), Cint, (Ptr{Cvoid},), s.h) != 0
"adopts a polee_loglik handle (DeviceSample's inner constructor always builds from CSC)"
function wrap_sample(h::Ptr{Cvoid}, ctx::Context, m, n)
    s = DeviceSampleHandle(h, ctx, Int(m), Int(n))
    finalizer(x -> ccall((:polee_loglik_destroy, LIB), Cvoid, (Ptr{Cvoid},), x.h), s)
    return s
end
mutable struct DeviceSampleHandle
    h::Ptr{Cvoid}
    ctx::Context
    m::Int
    n::Int
end
const AnySample = Union{DeviceSample,DeviceSampleHandle}

"X by columns on the device, uploaded once for the tree and the layout (polee_devx_upload): `sample_from_devx`, `hclust_from_devx`"
mutable struct DeviceX
    h::Ptr{Cvoid}
    ctx::Context
    m::Int
    n::Int
    function DeviceX(ctx::Context, m, n, colptr::Union{Vector{UInt32},Vector{UInt64}}, rowval::Vector{UInt32}, nzval::Vector{Float32})
        r = Ref{Ptr{Cvoid}}(C_NULL)
        GC.@preserve colptr rowval nzval check(
            ccall((:polee_devx_upload, LIB), Cint, (Ptr{Cvoid}, Int64, Int64, Ptr{Cvoid}, Cint, Ptr{UInt32}, Ptr{Float32}, Ref{Ptr{Cvoid}}),
                  ctx.h, m, n, colptr, sizeof(eltype(colptr)), rowval, isempty(nzval) ? C_NULL : pointer(nzval), r), ctx.h)
        x = new(r[], ctx, m, n)
        finalizer(x -> ccall((:polee_devx_destroy, LIB), Cvoid, (Ptr{Cvoid},), x.h), x)
        return x
    end
end
"the values after the fact (DeviceX(..., nzval) with an empty nzval uploads colptr + rowval only: enough for the tree)"
upload_values!(x::DeviceX, nzval::Vector{Float32}) =
    GC.@preserve nzval check(ccall((:polee_devx_upload_values, LIB), Cint, (Ptr{Cvoid}, Ptr{Float32}), x.h, nzval), x.ctx.h)
function sample_from_devx(ctx::Context, x::DeviceX; ks::Union{Nothing,Vector{Int64}}=nothing, nzval::Union{Nothing,Vector{Float32}}=nothing)
    r = Ref{Ptr{Cvoid}}(C_NULL)   # nzval: the values, if the handle has none yet (uploaded beside the layout's first kernels)
    GC.@preserve ks nzval check(ccall((:polee_loglik_create_from_devx, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float32}, Ptr{Int64}, Ref{Ptr{Cvoid}}),
                                      ctx.h, x.h, nzval === nothing ? C_NULL : nzval, ks === nothing ? C_NULL : ks, r), ctx.h)
    s = DeviceSampleHandle(r[], ctx, x.m, x.n)
    finalizer(s -> ccall((:polee_loglik_destroy, LIB), Cvoid, (Ptr{Cvoid},), s.h), s)
    return s
end
function hclust_from_devx(ctx::Context, x::DeviceX)
    parents, js = Vector{Int32}(undef, 2 * x.n - 1), Vector{Int32}(undef, 2 * x.n - 1)
    GC.@preserve parents js check(ccall((:polee_hclust_parallel_device_from_devx, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Int32}, Ptr{Int32}),
                                        ctx.h, x.h, parents, js), ctx.h)
    return parents, js
end

"mirror of `polee_loglik_info` (include/polee_hip.h): field order and types must stay in step with the header"
mutable struct LoglikInfo
    m::Int64; n::Int64; nnz::Int64; num_slices::Int64; num_tiles::Int64; padded_nnz::Int64
    device_bytes::Int64; stream_bytes::Int64; num_empty_rows::Int64; max_row_nnz::Int32; max_tile_cols::Int32
    stream_rows::NTuple{8,Int64}; stream_nnz::NTuple{8,Int64}; stream_tiles::NTuple{8,Int64}; stream_bytes_hbm::NTuple{8,Int64}
    dict_entries::Int64
    LoglikInfo() = new(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, ntuple(_ -> 0, 8), ntuple(_ -> 0, 8), ntuple(_ -> 0, 8), ntuple(_ -> 0, 8), 0)
end
function info(s::AnySample)
    i = LoglikInfo()
    check(ccall((:polee_loglik_get_info, LIB), Cint, (Ptr{Cvoid}, Ref{LoglikInfo}), s.h, i), s.ctx.h)
    return i
end
"bitwise reproducible gradient sums (fixed reduction order instead of float atomics)"
set_deterministic!(s::AnySample, on::Bool=true) =
    check(ccall((:polee_loglik_set_deterministic, LIB), Cint, (Ptr{Cvoid}, Cint), s.h, on), s.ctx.h)
"debug: every slice through the per-tile kernel (the second algorithm of the cross-check tests)"
debug_force_mixed!(s::AnySample, on::Bool=true) =
    check(ccall((:polee_debug_loglik_force_mixed, LIB), Cint, (Ptr{Cvoid}, Cint), s.h, on), s.ctx.h)

"K expression vectors at once: xs Float32 [n, K] (a column per draw) -> (lp [K], x_grad Float64 [n, K])"
function log_likelihood_batch(s::AnySample, xs::Matrix{Float32}; gradonly::Bool=false)
    K = size(xs, 2)
    g, lp = Matrix{Float64}(undef, size(xs, 1), K), Vector{Float64}(undef, K)
    GC.@preserve xs g lp check(
        ccall((:polee_loglik_eval, LIB), Cint, (Ptr{Cvoid}, Ptr{Float32}, Int32, Ptr{Float64}, Ptr{Float64}),
              s.h, xs, K, g, gradonly ? C_NULL : pointer(lp)), s.ctx.h)
    return lp, g
end

"OptimizePTTApprox (likelihood-approximation.jl:149-242): maximum-likelihood point estimate -> (xs, zs)"
function optimize_ptt(s::AnySample, t::AnyTree, efflens::Vector{Float32}, num_steps::Integer=500)
    xs, zs = Vector{Float32}(undef, s.n), Vector{Float32}(undef, s.n - 1)
    GC.@preserve efflens xs zs check(
        ccall((:polee_optimize_ptt, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float32}, Int32, Ptr{Float32}, Ptr{Float32}),
              s.h, t.h, efflens, num_steps, xs, zs), s.ctx.h)
    return xs, zs
end

# ---- the VI handle's test hooks ---------------------------------------------------------------------------------------
"""
One iteration's quantities WITHOUT applying the update (the parity tests' hook): K draws of the current parameters ->
(xs [n,K], x_grad [n,K], y_grad [n-1,K], mu_grad, omega_grad, alpha_grad [n-1], lp [K], ladj [K]).
"""
function eval_gradients(f::LikelihoodApproximationFit, K::Integer)
    n = f.t.n
    xs, xg, yg = Matrix{Float32}(undef, n, K), Matrix{Float64}(undef, n, K), Matrix{Float64}(undef, n - 1, K)
    mg, og, ag = (Vector{Float32}(undef, n - 1) for _ in 1:3)
    lp, ladj = Vector{Float64}(undef, K), Vector{Float64}(undef, K)
    GC.@preserve xs xg yg mg og ag lp ladj check(
        ccall((:polee_vi_eval_gradients, LIB), Cint,
              (Ptr{Cvoid}, Ptr{Float32}, Ptr{Float64}, Ptr{Float64}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Float64}, Ptr{Float64}),
              f.h, xs, xg, yg, mg, og, ag, lp, ladj), f.t.ctx.h)
    return xs, xg, yg, mg, og, ag, lp, ladj
end
"the N(0,1) draws iteration `step` uses (device RNG or the caller's table): Float32 [n-1, K]"
function export_noise(f::LikelihoodApproximationFit, step::Integer, K::Integer)
    z = Matrix{Float32}(undef, f.t.n - 1, K)
    GC.@preserve z check(ccall((:polee_vi_export_noise, LIB), Cint, (Ptr{Cvoid}, Int32, Ptr{Float32}), f.h, step, z), f.t.ctx.h)
    return z
end

# ---- communicators: what the transport reports; a host-side all-reduce through it ------------------------------------
const AnyComm = Union{Comm,HostComm}
comm_rank(c::AnyComm) = Int(ccall((:polee_comm_rank, LIB), Int32, (Ptr{Cvoid},), c.h))
comm_size(c::AnyComm) = Int(ccall((:polee_comm_size, LIB), Int32, (Ptr{Cvoid},), c.h))
"(transport, count, rank): transport 1 = RCCL (count / rank = ncclCommCount / ncclCommUserRank), 2 = host-staged"
function comm_info(c::AnyComm)
    t, n, r = Ref{Int32}(0), Ref{Int32}(0), Ref{Int32}(0)
    check(ccall((:polee_comm_info, LIB), Cint, (Ptr{Cvoid}, Ref{Int32}, Ref{Int32}, Ref{Int32}), c.h, t, n, r), c.ctx.h)
    return Int(t[]), Int(n[]), Int(r[])
end
"sum of a Float32 vector over the ranks, in place"
function allreduce_sum!(c::AnyComm, buf::Vector{Float32})
    GC.@preserve buf check(ccall((:polee_allreduce_sum_f32, LIB), Cint, (Ptr{Cvoid}, Ptr{Float32}, Int64), c.h, buf, length(buf)), c.ctx.h)
    return buf
end

# ---- density of the approximations on device buffers; splicing moments ------------------------------------------------
"as log_prob with DEVICE pointers (Ptr{Float32} into memory of the context's GPU): for callers with their own HIP code"
log_prob_device(ap::ApproxLikelihood, d_x::Ptr{Float32}, d_lp::Ptr{Float32}, d_x_grad::Ptr{Float32}=Ptr{Float32}(C_NULL)) =
    check(ccall((:polee_approx_logprob_device, LIB), Cint, (Ptr{Cvoid}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}), ap.h, d_x, d_lp, d_x_grad), ap.ctx.h)

"approximate_splicing_likelihood (polee_splicing.py:14-113): (loc, scale) Float32 [S*F]; index pairs (feature, transcript), 1-based, flattened"
function splicing_moments(ap::ApproxLikelihood, feature_indices::Vector{Int32}, antifeature_indices::Vector{Int32}, F::Integer;
                          num_mean_draws::Integer=1000, num_var_draws::Integer=1000, seed::Integer=0)
    loc, scale = Vector{Float32}(undef, ap.S * F), Vector{Float32}(undef, ap.S * F)
    GC.@preserve feature_indices antifeature_indices loc scale check(
        ccall((:polee_approx_splicing_moments, LIB), Cint,
              (Ptr{Cvoid}, Ptr{Int32}, Int64, Ptr{Int32}, Int64, Int32, Int32, Int32, UInt64, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}),
              ap.h, feature_indices, div(length(feature_indices), 2), antifeature_indices, div(length(antifeature_indices), 2), F,
              num_mean_draws, num_var_draws, seed, C_NULL, loc, scale), ap.ctx.h)
    return loc, scale
end

# ---- regression model: evaluation hook, parameter access, the Normal-likelihood variant --------------------------------
num_noise(r::Regression) = Int(ccall((:polee_regression_num_noise, LIB), Int64, (Ptr{Cvoid},), r.h))
"loss (and gradient with respect to the flat parameter vector) at one draw of the latents: the tests' hook"
function eval_loss(r::Regression; noise::Union{Nothing,Vector{Float32}}=nothing, seed::Integer=0, grad::Bool=false)
    loss = Ref{Float32}(0f0)
    g = grad ? Vector{Float32}(undef, num_params(r)) : Float32[]
    GC.@preserve noise g check(
        ccall((:polee_regression_eval, LIB), Cint, (Ptr{Cvoid}, Ptr{Float32}, UInt64, Ref{Float32}, Ptr{Float32}),
              r.h, noise === nothing ? C_NULL : pointer(noise), seed, loss, grad ? pointer(g) : C_NULL), r.ctx.h)
    return grad ? (loss[], g) : loss[]
end
function set_flat_params!(r::Regression, p::Vector{Float32})
    @assert length(p) == num_params(r)
    GC.@preserve p check(ccall((:polee_regression_set_params, LIB), Cint, (Ptr{Cvoid}, Ptr{Float32}), r.h, p), r.ctx.h)
end
function set_isoform_params!(r::Regression, p::Vector{Float32})
    GC.@preserve p check(ccall((:polee_regression_set_isoform_params, LIB), Cint, (Ptr{Cvoid}, Ptr{Float32}), r.h, p), r.ctx.h)
end
function isoform_grad(r::Regression)
    n = Int(ccall((:polee_regression_num_isoform_params, LIB), Int64, (Ptr{Cvoid},), r.h))
    g = Vector{Float32}(undef, n)
    GC.@preserve g check(ccall((:polee_regression_get_isoform_grad, LIB), Cint, (Ptr{Cvoid}, Ptr{Float32}), r.h, g), r.ctx.h)
    return g
end
"RNASeqNormalTranscriptLinearRegression (models/polee_regression.py:490-531): x ~ Normal(loc, scale) per sample, [S*n] row-major"
function set_normal_likelihood!(r::Regression, loc::Vector{Float32}, scale::Vector{Float32})
    GC.@preserve loc scale check(ccall((:polee_regression_set_normal_likelihood, LIB), Cint, (Ptr{Cvoid}, Ptr{Float32}, Ptr{Float32}), r.h, loc, scale), r.ctx.h)
end
# classify (models/polee_regression.py:342-413), the device part: the relaxed design rows of one step go in with set_design!, fit
# (one step) moves only the flat parameters [first, last] (1-based, inclusive; an empty range freezes them all), and
# design_gradient returns d loss / d design of the last evaluation.  The relaxed one-hot rows, their density and the logits' Adam are
# host arithmetic on S x F numbers (polee_amd/regression.py classify is the worked example).
function set_design!(r::Regression, design::Matrix{Float32})
    d = permutedims(design)  # C order [S][F]
    GC.@preserve d check(ccall((:polee_regression_set_design, LIB), Cint, (Ptr{Cvoid}, Ptr{Float32}), r.h, d), r.ctx.h)
end
function set_trainable!(r::Regression, first::Integer, last::Integer)
    check(ccall((:polee_regression_set_trainable, LIB), Cint, (Ptr{Cvoid}, Int64, Int64), r.h, Int64(first - 1), Int64(last)), r.ctx.h)
end
function design_gradient(r::Regression, S::Integer, F::Integer)
    g = Matrix{Float32}(undef, F, S)
    GC.@preserve g check(ccall((:polee_regression_design_grad, LIB), Cint, (Ptr{Cvoid}, Ptr{Float32}), r.h, g), r.ctx.h)
    return permutedims(g)
end
# RNASeqPCA (models/polee_pca.py:14-92), the device part: the design matrix becomes a trained latent z [S x F] with a Normal(0,
# prior_scale) prior and a point surrogate; fit! then trains it on the device with the flat parameters, and design_gradient returns the
# total d loss / dz (prior term included).  get_design returns the current z (any handle: its design matrix).
function set_latent_design!(r::Regression, z0::Matrix{Float32}, prior_scale::Real=1.0)
    z = permutedims(z0)  # C order [S][F]
    GC.@preserve z check(ccall((:polee_regression_set_latent_design, LIB), Cint, (Ptr{Cvoid}, Ptr{Float32}, Cfloat), r.h, z, Float32(prior_scale)), r.ctx.h)
end
function get_design(r::Regression, S::Integer, F::Integer)
    d = Matrix{Float32}(undef, F, S)
    GC.@preserve d check(ccall((:polee_regression_get_design, LIB), Cint, (Ptr{Cvoid}, Ptr{Float32}), r.h, d), r.ctx.h)
    return permutedims(d)
end

"the kernel-regression weights of the mean-variance prior, Float32 [degree*n] (models/polee_regression.py:436-460)"
function regression_weights(r::Regression, degree::Integer=15)
    w = Vector{Float32}(undef, degree * r.n)
    GC.@preserve w check(ccall((:polee_regression_weights, LIB), Cint, (Ptr{Cvoid}, Ptr{Float32}), r.h, w), r.ctx.h)
    return w
end

# ---- X construction (src/rnaseq_sample.jl:390-524 with the SimplisticFragModel, src/fragmodel.jl:23-169) --------------
struct XbTranscripts
    n::Int32; seq::Ptr{Int32}; strand::Ptr{Int8}; exon_ptr::Ptr{Int64}; exon_first::Ptr{Int64}; exon_last::Ptr{Int64}
end
struct XbFragments
    m::Int64; seq::Ptr{Int32}; strand::Ptr{Int8}
    m1_left::Ptr{Int64}; m1_right::Ptr{Int64}; m2_left::Ptr{Int64}; m2_right::Ptr{Int64}
    m1_is_flag16::Ptr{UInt8}; cig1_ptr::Ptr{Int64}; cig2_ptr::Ptr{Int64}; cig_op::Ptr{UInt8}; cig_len::Ptr{Int32}
end
struct XbFragModel
    fraglen_pmf::Ptr{Float32}; fraglen_cdf::Ptr{Float32}; fraglen_median::Int32; strand_specificity::Float32; alt_frag_model::Int32
end
"""
    build_likelihood_matrix(ctx, T, F, pmf, cdf, median; strand_specificity, alt_frag_model)

T: NamedTuple (seq, strand, exon_ptr, exon_first, exon_last), F: NamedTuple (seq, strand, m1_left, m1_right, m2_left,
m2_right, m1_is_flag16, cig1_ptr, cig2_ptr, cig_op, cig_len) in the layout of include/polee_hip.h (m1 = the LEFTMOST mate,
as transcripts.jl:288-297 orders them).  Returns (tcolptr, trowval, tnzval, effective_lengths, row_fragment): the rows of X.
"""
function build_likelihood_matrix(ctx::Context, T, F, pmf::Vector{Float32}, cdf::Vector{Float32}, median::Integer;
                                 strand_specificity::Real=0.9, alt_frag_model::Bool=false, return_sample::Bool=false, return_tree::Bool=false)
    n = length(T.seq); m = length(F.seq)
    out = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve T F pmf cdf begin
        ts = XbTranscripts(n, pointer(T.seq), pointer(T.strand), pointer(T.exon_ptr), pointer(T.exon_first), pointer(T.exon_last))
        fs = XbFragments(m, pointer(F.seq), pointer(F.strand), pointer(F.m1_left), pointer(F.m1_right), pointer(F.m2_left),
                         pointer(F.m2_right), pointer(F.m1_is_flag16), pointer(F.cig1_ptr), pointer(F.cig2_ptr), pointer(F.cig_op),
                         pointer(F.cig_len))
        ms = XbFragModel(pointer(pmf), pointer(cdf), median, strand_specificity, alt_frag_model)
        check(ccall((:polee_xbuild_run, LIB), Cint, (Ptr{Cvoid}, Ref{XbTranscripts}, Ref{XbFragments}, Ref{XbFragModel}, Ref{Ptr{Cvoid}}),
                    ctx.h, ts, fs, ms, out), ctx.h)
    end
    h = out[]
    try
        rows, nnz = Ref{Int64}(0), Ref{Int64}(0)
        check(ccall((:polee_xbuild_sizes, LIB), Cint, (Ptr{Cvoid}, Ref{Int64}, Ref{Int64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                    h, rows, nnz, C_NULL, C_NULL, C_NULL), ctx.h)
        tcolptr, trowval, tnzval = Vector{UInt64}(undef, rows[] + 1), Vector{UInt32}(undef, nnz[]), Vector{Float32}(undef, nnz[])
        efflens, rowfrag = Vector{Float32}(undef, n), Vector{Int64}(undef, rows[])
        GC.@preserve tcolptr trowval tnzval efflens rowfrag check(
            ccall((:polee_xbuild_get, LIB), Cint, (Ptr{Cvoid}, Ptr{UInt64}, Ptr{UInt32}, Ptr{Float32}, Ptr{Float32}, Ptr{Int64}),
                  h, tcolptr, trowval, tnzval, efflens, rowfrag), ctx.h)
        if return_tree   # the clustering tree (rounds variant) from the result on the device
            parents, js = Vector{Int32}(undef, 2n - 1), Vector{Int32}(undef, 2n - 1)
            GC.@preserve parents js check(ccall((:polee_hclust_parallel_device_from_xbuild, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Int32}, Ptr{Int32}),
                                                ctx.h, h, parents, js), ctx.h)
            return tcolptr, trowval, tnzval, efflens, rowfrag, parents, js
        end
        if return_sample  # the likelihood handle straight from the result on the device (X never visits the host on its way in)
            r = Ref{Ptr{Cvoid}}(C_NULL)
            check(ccall((:polee_loglik_create_from_xbuild, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Int64}, Ref{Ptr{Cvoid}}), ctx.h, h, C_NULL, r), ctx.h)
            return tcolptr, trowval, tnzval, efflens, rowfrag, wrap_sample(r[], ctx, rows[], n)
        end
        return tcolptr, trowval, tnzval, efflens, rowfrag
    finally
        ccall((:polee_xbuild_destroy, LIB), Cvoid, (Ptr{Cvoid},), h)
    end
end

# ---- the same under the BiasedFragModel (src/fragmodel.jl:174-445 with a TRAINED bias model; training stays upstream) ----------
struct XbBiasModel
    tseq_ptr::Ptr{Int64}; tseq::Ptr{UInt8}; seqbias_len::Int32; ps_ctx::Int32
    orders_left::Ptr{Int32}; orders_right::Ptr{Int32}; ps_left::Ptr{Float32}; ps_right::Ptr{Float32}
    gc_nbins::Int32; gc_bins::Ptr{Float32}; pos_p::Float64; pos_terms::Ptr{Float64}; pos_maxtlen::Int32
    num_fraglens::Int32; high_prob_fraglens::Ptr{Int32}; m1_reverse::Ptr{UInt8}
end
"""
    build_likelihood_matrix_biased(ctx, T, F, pmf, cdf, median, B; strand_specificity, alt_frag_model, return_bias)

As build_likelihood_matrix with the reference's default BiasedFragModel (polee_xbuild_run_biased): B is a NamedTuple in the layout of
polee_xb_biasmodel (include/polee_hip.h): tseq_ptr, tseq (0 A, 1 C, 2 G, 3 T, 4 other), orders_left / orders_right (Int32 [20], -1 =
position not in the model), ps_left / ps_right (Float32 [20][4][ps_ctx] row-major), gc_bins, high_prob_fraglens, and optionally
pos_p / pos_terms (PositionalBiasModel; `nothing` = use_pos_bias false) and m1_reverse (`nothing` when every fragment is paired).
Returns (tcolptr, trowval, tnzval, effective_lengths, row_fragment) and, with return_bias, the transcripts' left / right bias
vectors (polee_xbuild_get_bias, laid out like tseq).
"""
function build_likelihood_matrix_biased(ctx::Context, T, F, pmf::Vector{Float32}, cdf::Vector{Float32}, median::Integer, B;
                                        strand_specificity::Real=0.9, alt_frag_model::Bool=false, return_bias::Bool=false)
    n = length(T.seq); m = length(F.seq)
    out = Ref{Ptr{Cvoid}}(C_NULL)
    pos_terms = get(B, :pos_terms, nothing); m1_reverse = get(B, :m1_reverse, nothing)
    ps_ctx = div(length(B.ps_left), 20 * 4)
    GC.@preserve T F pmf cdf B pos_terms m1_reverse begin
        ts = XbTranscripts(n, pointer(T.seq), pointer(T.strand), pointer(T.exon_ptr), pointer(T.exon_first), pointer(T.exon_last))
        fs = XbFragments(m, pointer(F.seq), pointer(F.strand), pointer(F.m1_left), pointer(F.m1_right), pointer(F.m2_left),
                         pointer(F.m2_right), pointer(F.m1_is_flag16), pointer(F.cig1_ptr), pointer(F.cig2_ptr), pointer(F.cig_op),
                         pointer(F.cig_len))
        ms = XbFragModel(pointer(pmf), pointer(cdf), median, strand_specificity, alt_frag_model)
        bm = XbBiasModel(pointer(B.tseq_ptr), pointer(B.tseq), 20, ps_ctx, pointer(B.orders_left), pointer(B.orders_right),
                         pointer(B.ps_left), pointer(B.ps_right), length(B.gc_bins), pointer(B.gc_bins),
                         pos_terms === nothing ? 0.0 : Float64(B.pos_p), pos_terms === nothing ? Ptr{Float64}(C_NULL) : pointer(pos_terms),
                         pos_terms === nothing ? 0 : length(pos_terms), length(B.high_prob_fraglens), pointer(B.high_prob_fraglens),
                         m1_reverse === nothing ? Ptr{UInt8}(C_NULL) : pointer(m1_reverse))
        check(ccall((:polee_xbuild_run_biased, LIB), Cint,
                    (Ptr{Cvoid}, Ref{XbTranscripts}, Ref{XbFragments}, Ref{XbFragModel}, Ref{XbBiasModel}, Ref{Ptr{Cvoid}}),
                    ctx.h, ts, fs, ms, bm, out), ctx.h)
    end
    h = out[]
    try
        rows, nnz = Ref{Int64}(0), Ref{Int64}(0)
        check(ccall((:polee_xbuild_sizes, LIB), Cint, (Ptr{Cvoid}, Ref{Int64}, Ref{Int64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                    h, rows, nnz, C_NULL, C_NULL, C_NULL), ctx.h)
        tcolptr, trowval, tnzval = Vector{UInt64}(undef, rows[] + 1), Vector{UInt32}(undef, nnz[]), Vector{Float32}(undef, nnz[])
        efflens, rowfrag = Vector{Float32}(undef, n), Vector{Int64}(undef, rows[])
        GC.@preserve tcolptr trowval tnzval efflens rowfrag check(
            ccall((:polee_xbuild_get, LIB), Cint, (Ptr{Cvoid}, Ptr{UInt64}, Ptr{UInt32}, Ptr{Float32}, Ptr{Float32}, Ptr{Int64}),
                  h, tcolptr, trowval, tnzval, efflens, rowfrag), ctx.h)
        if return_bias
            len = Int(B.tseq_ptr[end])
            left, right = Vector{Float32}(undef, len), Vector{Float32}(undef, len)
            GC.@preserve left right check(ccall((:polee_xbuild_get_bias, LIB), Cint, (Ptr{Cvoid}, Ptr{Float32}, Ptr{Float32}, Ptr{Float64}),
                                                h, left, right, C_NULL), ctx.h)
            return tcolptr, trowval, tnzval, efflens, rowfrag, left, right
        end
        return tcolptr, trowval, tnzval, efflens, rowfrag
    finally
        ccall((:polee_xbuild_destroy, LIB), Cvoid, (Ptr{Cvoid},), h)
    end
end

# ---- the fragment model from the alignment pairs themselves (DESIGN.md section 3.18) ---------------------------------------------
"""
    fragmodel_estimate(ctx, T, F; min_fraglen=false)

The counts of SimplisticFragModel(rs, ts) (src/fragmodel.jl:35-67; polee_fragmodel_estimate): (counts, hist[, min_fraglen]) with
counts = [compatible pairs, strand matches, strand mismatches, fragments longer than 2000] and hist[l] = fragments whose smallest
positive length is l.  T, F as build_likelihood_matrix takes them.
"""
function fragmodel_estimate(ctx::Context, T, F; min_fraglen::Bool=false)
    n = length(T.seq); m = length(F.seq)
    counts, hist = zeros(Int64, 4), zeros(Int64, 2000)
    mins = min_fraglen ? zeros(Int64, m) : nothing
    GC.@preserve T F counts hist mins begin
        ts = XbTranscripts(n, pointer(T.seq), pointer(T.strand), pointer(T.exon_ptr), pointer(T.exon_first), pointer(T.exon_last))
        fs = XbFragments(m, pointer(F.seq), pointer(F.strand), pointer(F.m1_left), pointer(F.m1_right), pointer(F.m2_left),
                         pointer(F.m2_right), pointer(F.m1_is_flag16), pointer(F.cig1_ptr), pointer(F.cig2_ptr), pointer(F.cig_op),
                         pointer(F.cig_len))
        check(ccall((:polee_fragmodel_estimate, LIB), Cint, (Ptr{Cvoid}, Ref{XbTranscripts}, Ref{XbFragments}, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}),
                    ctx.h, ts, fs, counts, hist, mins === nothing ? Ptr{Int64}(C_NULL) : pointer(mins)), ctx.h)
    end
    return min_fraglen ? (counts, hist, mins) : (counts, hist)
end

"""
    read_assign(ctx, T, F, pmf, cdf, median, tseq_ptr, xs; strand_specificity, alt_frag_model, m1_reverse, seed, mode, fallback_fraglen)

X of the fragments under the SimplisticFragModel (polee_xbuild_run), then one transcript per row and the fragment's interval on it
(polee_read_assign; src/rnaseq_sample.jl:346-373, src/transcripts.jl:452-517).  mode 0: drawn in proportion to xs[j] X[i, j]; mode 1: the
last entry of every row, as the reference is written.  Returns (row_fragment, transcript (0-based), tpos, fraglen, flags).
"""
function read_assign(ctx::Context, T, F, pmf::Vector{Float32}, cdf::Vector{Float32}, median::Integer, tseq_ptr::Vector{Int64},
                     xs::Vector{Float32}; strand_specificity::Real=0.9, alt_frag_model::Bool=false, m1_reverse=nothing, seed::Integer=0,
                     mode::Integer=0, fallback_fraglen::Integer=150)
    n = length(T.seq); m = length(F.seq)
    out = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve T F pmf cdf tseq_ptr xs m1_reverse begin
        ts = XbTranscripts(n, pointer(T.seq), pointer(T.strand), pointer(T.exon_ptr), pointer(T.exon_first), pointer(T.exon_last))
        fs = XbFragments(m, pointer(F.seq), pointer(F.strand), pointer(F.m1_left), pointer(F.m1_right), pointer(F.m2_left),
                         pointer(F.m2_right), pointer(F.m1_is_flag16), pointer(F.cig1_ptr), pointer(F.cig2_ptr), pointer(F.cig_op),
                         pointer(F.cig_len))
        ms = XbFragModel(pointer(pmf), pointer(cdf), median, strand_specificity, alt_frag_model)
        check(ccall((:polee_xbuild_run, LIB), Cint, (Ptr{Cvoid}, Ref{XbTranscripts}, Ref{XbFragments}, Ref{XbFragModel}, Ref{Ptr{Cvoid}}),
                    ctx.h, ts, fs, ms, out), ctx.h)
        h = out[]
        try
            rows = Ref{Int64}(0)
            check(ccall((:polee_xbuild_sizes, LIB), Cint, (Ptr{Cvoid}, Ref{Int64}, Ptr{Int64}, Ptr{Float64}, Ptr{Float64}, Ptr{Float64}),
                        h, rows, C_NULL, C_NULL, C_NULL, C_NULL), ctx.h)
            rowfrag, transcript, tpos = Vector{Int64}(undef, rows[]), Vector{Int32}(undef, rows[]), Vector{Int64}(undef, rows[])
            fraglen, flags = Vector{Int32}(undef, rows[]), Vector{UInt8}(undef, rows[])
            GC.@preserve rowfrag transcript tpos fraglen flags begin
                check(ccall((:polee_xbuild_get, LIB), Cint, (Ptr{Cvoid}, Ptr{UInt64}, Ptr{UInt32}, Ptr{Float32}, Ptr{Float32}, Ptr{Int64}),
                            h, C_NULL, C_NULL, C_NULL, C_NULL, rowfrag), ctx.h)
                check(ccall((:polee_read_assign, LIB), Cint,
                            (Ptr{Cvoid}, Ptr{Cvoid}, Ref{XbTranscripts}, Ref{XbFragments}, Ptr{Int64}, Ptr{UInt8}, Ptr{Float32}, UInt64, Int32, Int32,
                             Ptr{Int32}, Ptr{Int64}, Ptr{Int32}, Ptr{UInt8}),
                            ctx.h, h, ts, fs, tseq_ptr, m1_reverse === nothing ? Ptr{UInt8}(C_NULL) : pointer(m1_reverse), xs, UInt64(seed), mode,
                            fallback_fraglen, transcript, tpos, fraglen, flags), ctx.h)
            end
            return rowfrag, transcript, tpos, fraglen, flags
        finally
            ccall((:polee_xbuild_destroy, LIB), Cvoid, (Ptr{Cvoid},), h)
        end
    end
end

"fast_log of the tree kernels (csrc/scan.hpp), element-wise on the device: the tests compare it with Base.log"
function debug_fast_log(ctx::Context, x::Vector{Float64})
    out = similar(x)
    GC.@preserve x out check(ccall((:polee_debug_fast_log, LIB), Cint, (Ptr{Cvoid}, Ptr{Float64}, Int64, Ptr{Float64}), ctx.h, x, length(x), out), ctx.h)
    return out
end

# ---- Gibbs sampler of the exact posterior (src/gibbs.jl; `polee debug-sample`, main.jl:925-957) -------------------------------
mutable struct GibbsSampler
    h::Ptr{Cvoid}
    ctx::Context
    n::Int
    num_chains::Int
end

struct GibbsInfo
    m::Int64; n::Int64; nnz::Int64
    num_chains::Int32
    num_multi_rows::Int64; num_single_rows::Int64; num_empty_rows::Int64; multi_nnz::Int64; num_tiles::Int64
    rows_per_tile::Int32
    sweeps_done::Int64
end

function wrap_gibbs(r::Ref{Ptr{Cvoid}}, ctx::Context, n, num_chains)
    g = GibbsSampler(r[], ctx, Int(n), Int(num_chains))
    finalizer(x -> ccall((:polee_gibbs_destroy, LIB), Cvoid, (Ptr{Cvoid},), x.h), g)
    return g
end

"X by columns exactly as RNASeqSample holds it (colptr, rowval 1-based); efflens === nothing = --no-efflen"
function GibbsSampler(ctx::Context, m::Integer, n::Integer, colptr::Vector{UInt32}, rowval::Vector{UInt32}, nzval::Vector{Float32},
                      efflens::Union{Nothing,Vector{Float32}}, num_chains::Integer, seed::Integer)
    r = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve colptr rowval nzval efflens check(
        ccall((:polee_gibbs_create, LIB), Cint,
              (Ptr{Cvoid}, Int64, Int64, Ptr{Cvoid}, Cint, Ptr{UInt32}, Ptr{Float32}, Ptr{Float32}, Int32, UInt64, Ref{Ptr{Cvoid}}),
              ctx.h, m, n, colptr, 4, rowval, nzval, efflens === nothing ? C_NULL : pointer(efflens), num_chains, UInt64(seed), r), ctx.h)
    return wrap_gibbs(r, ctx, n, num_chains)
end

"X given fragment-major (Xt = SparseMatrixCSC(transpose(X)), as gibbs.jl:26 builds it)"
function gibbs_sampler_from_xt(ctx::Context, m::Integer, n::Integer, tcolptr::Vector{UInt64}, trowval::Vector{UInt32},
                               tnzval::Vector{Float32}, efflens::Union{Nothing,Vector{Float32}}, num_chains::Integer, seed::Integer)
    r = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve tcolptr trowval tnzval efflens check(
        ccall((:polee_gibbs_create_from_xt, LIB), Cint,
              (Ptr{Cvoid}, Int64, Int64, Ptr{UInt64}, Ptr{UInt32}, Ptr{Float32}, Ptr{Float32}, Int32, UInt64, Ref{Ptr{Cvoid}}),
              ctx.h, m, n, tcolptr, trowval, tnzval, efflens === nothing ? C_NULL : pointer(efflens), num_chains, UInt64(seed), r), ctx.h)
    return wrap_gibbs(r, ctx, n, num_chains)
end

"g0: [n, C] (column c = chain c's unnormalised mixture), or nothing = fresh Gamma(1) draws"
function set_state!(g::GibbsSampler, g0::Union{Nothing,Matrix{Float32}})
    GC.@preserve g0 check(ccall((:polee_gibbs_set_state, LIB), Cint, (Ptr{Cvoid}, Ptr{Float32}), g.h,
                                g0 === nothing ? C_NULL : pointer(g0)), g.ctx.h)
end
reserve!(g::GibbsSampler, draws_per_chain::Integer) =
    check(ccall((:polee_gibbs_reserve, LIB), Cint, (Ptr{Cvoid}, Int32), g.h, draws_per_chain), g.ctx.h)
"nsweeps sweeps; stride > 0 stores every stride-th state, 0 = burn-in"
run!(g::GibbsSampler, nsweeps::Integer, stride::Integer=0) =
    check(ccall((:polee_gibbs_run, LIB), Cint, (Ptr{Cvoid}, Int32, Int32), g.h, nsweeps, stride), g.ctx.h)
sync!(g::GibbsSampler) = check(ccall((:polee_gibbs_sync, LIB), Cint, (Ptr{Cvoid},), g.h), g.ctx.h)
function num_stored(g::GibbsSampler)
    k = Ref{Int32}(0)
    check(ccall((:polee_gibbs_num_stored, LIB), Cint, (Ptr{Cvoid}, Ref{Int32}), g.h, k), g.ctx.h)
    return Int(k[])
end
"stored draws first+1 .. first+count: [n, count, C] (the samples array of gibbs.jl:71, dimensions reversed)"
function get_draws(g::GibbsSampler, first::Integer=0, count::Integer=num_stored(g) - first)
    out = Array{Float32}(undef, g.n, count, g.num_chains)
    GC.@preserve out check(ccall((:polee_gibbs_get_draws, LIB), Cint, (Ptr{Cvoid}, Int32, Int32, Ptr{Float32}),
                                 g.h, first, count, out), g.ctx.h)
    return out
end
function get_counts(g::GibbsSampler)
    out = Matrix{UInt32}(undef, g.n, g.num_chains)
    GC.@preserve out check(ccall((:polee_gibbs_get_counts, LIB), Cint, (Ptr{Cvoid}, Ptr{UInt32}), g.h, out), g.ctx.h)
    return out
end
"split-R-hat per transcript over all stored draws (convergence_stats, gibbs.jl:283-319)"
function rhat(g::GibbsSampler)
    out = Vector{Float32}(undef, g.n)
    GC.@preserve out check(ccall((:polee_gibbs_rhat, LIB), Cint, (Ptr{Cvoid}, Ptr{Float32}), g.h, out), g.ctx.h)
    return out
end
function info(g::GibbsSampler)
    i = Ref{GibbsInfo}()
    check(ccall((:polee_gibbs_get_info, LIB), Cint, (Ptr{Cvoid}, Ref{GibbsInfo}), g.h, i), g.ctx.h)
    return i[]
end
"test hook: the 1-based transcript the last sweep gave each fragment, chain `chain` (0-based), 0 = empty fragment"
function debug_gibbs_assignments(g::GibbsSampler, chain::Integer, m::Integer)
    z = Vector{Int32}(undef, m)
    GC.@preserve z check(ccall((:polee_debug_gibbs_assignments, LIB), Cint, (Ptr{Cvoid}, Int32, Ptr{Int32}), g.h, chain, z), g.ctx.h)
    return z
end

# ---- EM maximum-likelihood estimate (src/em.jl:3-87; `polee debug-optimize`, main.jl:960-988) ----------------------------------
mutable struct EM
    h::Ptr{Cvoid}
    sample::AnySample   # kept alive: the handle works on the sample's X
    n::Int
end

"mirror of `polee_em_info` (include/polee_hip.h): field order and types must stay in step with the header"
struct EMInfo
    n::Int64; M::Int64; iters::Int64
    converged::Int32; nonfinite::Int32
    lp_start::Float64; last_lp::Float64; last_increase::Float64; sum_y::Float64; kkt_max::Float64
end

"EM over the X of an existing device sample; y0 === nothing: the reference's start 1/n (em.jl:22).  While iterations run, nothing
else may evaluate the same sample (one evaluation slot per likelihood handle)."
function EM(s::AnySample, y0::Union{Nothing,Vector{Float32}}=nothing)
    r = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve y0 check(ccall((:polee_em_create, LIB), Cint, (Ptr{Cvoid}, Ptr{Float32}, Ref{Ptr{Cvoid}}),
                                s.h, y0 === nothing ? C_NULL : pointer(y0), r), s.ctx.h)
    em = EM(r[], s, Int(s.n))
    finalizer(x -> ccall((:polee_em_destroy, LIB), Cvoid, (Ptr{Cvoid},), x.h), em)
    return em
end
function reset!(em::EM, y0::Union{Nothing,Vector{Float32}}=nothing)
    GC.@preserve y0 check(ccall((:polee_em_reset, LIB), Cint, (Ptr{Cvoid}, Ptr{Float32}), em.h,
                                y0 === nothing ? C_NULL : pointer(y0)), em.sample.ctx.h)
end
"up to max_iters more iterations; stops with the first iterate whose log-likelihood gains less than tol (em.jl:76; tol < 0: never)"
run!(em::EM, max_iters::Integer=5000, tol::Real=1e-6, check_every::Integer=64) =
    check(ccall((:polee_em_run, LIB), Cint, (Ptr{Cvoid}, Int32, Float64, Int32), em.h, max_iters, tol, check_every), em.sample.ctx.h)
sync!(em::EM) = check(ccall((:polee_em_sync, LIB), Cint, (Ptr{Cvoid},), em.h), em.sample.ctx.h)
function mixture(em::EM)
    y = Vector{Float32}(undef, em.n)
    GC.@preserve y check(ccall((:polee_em_get_mixture, LIB), Cint, (Ptr{Cvoid}, Ptr{Float32}), em.h, y), em.sample.ctx.h)
    return y
end
"1e6 (y / efflens) / sum(y / efflens) (em.jl:82-84); efflens === nothing: 1e6 y"
function tpm(em::EM, efflens::Union{Nothing,Vector{Float32}})
    out = Vector{Float32}(undef, em.n)
    GC.@preserve efflens out check(ccall((:polee_em_get_tpm, LIB), Cint, (Ptr{Cvoid}, Ptr{Float32}, Ptr{Float32}), em.h,
                                         efflens === nothing ? C_NULL : pointer(efflens), out), em.sample.ctx.h)
    return out
end
"log-likelihood of iterates 1, 2, ... (the reference's `@show lp`, em.jl:74)"
function trace(em::EM)
    k = Ref{Int64}(0)
    check(ccall((:polee_em_get_trace, LIB), Cint, (Ptr{Cvoid}, Ptr{Float64}, Int64, Ref{Int64}), em.h, C_NULL, 0, k), em.sample.ctx.h)
    lp = Vector{Float64}(undef, k[])
    GC.@preserve lp check(ccall((:polee_em_get_trace, LIB), Cint, (Ptr{Cvoid}, Ptr{Float64}, Int64, Ref{Int64}), em.h, lp, length(lp), k),
                          em.sample.ctx.h)
    return lp
end
"kkt = true: the fixed-point residual max_j y_j |g_j / M - 1| of the mixture handed out, from an f64 gradient pass of its own"
function info(em::EM; kkt::Bool=false)
    i = Ref{EMInfo}()
    check(ccall((:polee_em_get_info, LIB), Cint, (Ptr{Cvoid}, Cint, Ref{EMInfo}), em.h, kkt ? 1 : 0, i), em.sample.ctx.h)
    return i[]
end
"expectation_maximization (em.jl:3-87) on a device sample: the TPM vector"
function expectation_maximization(s::AnySample, efflens::Union{Nothing,Vector{Float32}}; max_iters::Integer=5000, tol::Real=1e-6)
    em = EM(s)
    run!(em, max_iters, tol)
    return tpm(em, efflens)
end

# ---- `polee sample` (main.jl:756-919): streamed draws, posterior mean, prop_to_counts, exact multinomial counts ------------------
mutable struct SampleStream
    h::Ptr{Cvoid}
    t::PolyaTreeTransform   # kept alive: the handle uses the tree and its scratch
    n::Int
end

"a stream of draws from one fitted approximation; sigma = exp.(omega); 0 <= m < 2^31"
function SampleStream(t::PolyaTreeTransform, mu::Vector{Float32}, sigma::Vector{Float32}, alpha::Vector{Float32},
                      efflens::Vector{Float32}, m::Integer; seed::Integer=123456789)
    r = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve mu sigma alpha efflens check(
        ccall((:polee_sampler_create, LIB), Cint,
              (Ptr{Cvoid}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Int64, UInt64, Ref{Ptr{Cvoid}}),
              t.h, mu, sigma, alpha, efflens, m, seed, r), t.ctx.h)
    s = SampleStream(r[], t, length(efflens))
    finalizer(x -> ccall((:polee_sampler_destroy, LIB), Cvoid, (Ptr{Cvoid},), x.h), s)
    return s
end
"the next `count` draws: (props n x count Float32, counts n x count Float64 or nothing); sample_counts: exact multinomial counts
(--sample-counts) instead of expected ones (main.jl:859-880).  Columns are draws."
function next!(s::SampleStream, count::Integer; counts::Bool=true, sample_counts::Bool=false)
    props = Matrix{Float32}(undef, s.n, count)
    cs = counts ? Matrix{Float64}(undef, s.n, count) : nothing
    GC.@preserve props cs check(
        ccall((:polee_sampler_next, LIB), Cint,
              (Ptr{Cvoid}, Int32, Int32, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Float64}),
              s.h, count, sample_counts ? 1 : 0, C_NULL, C_NULL, props, cs === nothing ? C_NULL : pointer(cs)), s.t.ctx.h)
    return props, cs
end
function num_draws(s::SampleStream)
    k = Ref{Int64}(0)
    check(ccall((:polee_sampler_num_draws, LIB), Cint, (Ptr{Cvoid}, Ref{Int64}), s.h, k), s.t.ctx.h)
    return k[]
end
"(post_mean, est_counts = prop_to_counts(post_mean)) of all draws so far (main.jl:857, :887)"
function posterior_mean(s::SampleStream; sample_counts::Bool=false)
    pm = Vector{Float32}(undef, s.n); ec = Vector{Float64}(undef, s.n)
    GC.@preserve pm ec check(ccall((:polee_sampler_mean, LIB), Cint, (Ptr{Cvoid}, Ptr{Float32}, Ptr{Float64}, Int32),
                                   s.h, pm, ec, sample_counts ? 1 : 0), s.t.ctx.h)
    return pm, ec
end
"exact multinomial draws of m items: p is n x D (a column = the shares of one draw, >= 0, not necessarily normalised) -> n x D
UInt32 counts, every column summing to m; column r is draw first_draw + r - 1, a pure function of (shares, m, seed, draw index)"
function multinomial_counts(ctx::Context, p::Matrix{Float64}, m::Integer; seed::Integer=123456789, first_draw::Integer=0)
    out = Matrix{UInt32}(undef, size(p, 1), size(p, 2))
    GC.@preserve p out check(
        ccall((:polee_multinomial_counts, LIB), Cint, (Ptr{Cvoid}, Ptr{Float64}, Int32, Int64, Int64, UInt64, UInt64, Ptr{UInt32}),
              ctx.h, p, size(p, 2), size(p, 1), m, seed, first_draw, out), ctx.h)
    return out
end

# ---- `polee model classify` (models/classify.jl, models/polee_classify.py:13-114): logistic regression on posterior draws -----------
"mirror of `polee_classify_opts` (include/polee_hip.h): field order and types must stay in step with the header"
mutable struct ClassifyOpts
    draws_per_step::Int32
    learning_rate::Float32; l1_penalty::Float32; loss_scale::Float32
    beta1::Float32; beta2::Float32; epsilon::Float32
    function ClassifyOpts()
        o = new()
        ccall((:polee_classify_default_opts, LIB), Cvoid, (Ref{ClassifyOpts},), o)
        return o
    end
end

"RNASeqLogisticRegression (polee_classify.py:13-20); matrices are row-major vectors: w [n*k] (transcript by transcript), labels and
probabilities [S*k] (sample by sample)"
mutable struct LogisticRegression
    h::Ptr{Cvoid}
    ctx::Context
    n::Int
    k::Int
end
function LogisticRegression(ctx::Context, k::Integer, n::Integer; opts::ClassifyOpts=ClassifyOpts())
    r = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:polee_classify_create, LIB), Cint, (Ptr{Cvoid}, Int32, Int32, Ref{ClassifyOpts}, Ref{Ptr{Cvoid}}), ctx.h, n, k, opts, r),
          ctx.h)
    cl = LogisticRegression(r[], ctx, n, k)
    finalizer(x -> ccall((:polee_classify_destroy, LIB), Cvoid, (Ptr{Cvoid},), x.h), cl)
    return cl
end
set_opts!(cl::LogisticRegression, opts::ClassifyOpts) =
    check(ccall((:polee_classify_set_opts, LIB), Cint, (Ptr{Cvoid}, Ref{ClassifyOpts}), cl.h, opts), cl.ctx.h)
"(w [n*k], x_bias [n], z_bias [k])"
function get_params(cl::LogisticRegression)
    w = Vector{Float32}(undef, cl.n * cl.k); xb = Vector{Float32}(undef, cl.n); zb = Vector{Float32}(undef, cl.k)
    GC.@preserve w xb zb check(ccall((:polee_classify_get_params, LIB), Cint, (Ptr{Cvoid}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}),
                                     cl.h, w, xb, zb), cl.ctx.h)
    return w, xb, zb
end
function set_params!(cl::LogisticRegression, w::Vector{Float32}, x_bias::Vector{Float32}, z_bias::Vector{Float32})
    GC.@preserve w x_bias z_bias check(ccall((:polee_classify_set_params, LIB), Cint,
                                             (Ptr{Cvoid}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}), cl.h, w, x_bias, z_bias), cl.ctx.h)
end
"Adam moments and step clock back to zero"
reset!(cl::LogisticRegression) = check(ccall((:polee_classify_reset, LIB), Cint, (Ptr{Cvoid},), cl.h), cl.ctx.h)
"x_bias <- column mean of the log of one draw (polee_classify.py:52-55)"
function init_bias!(cl::LogisticRegression, ap::ApproxLikelihood; seed::Integer=0, z0::Union{Nothing,Vector{Float32}}=nothing)
    GC.@preserve z0 check(ccall((:polee_classify_init_bias, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float32}, UInt64), cl.h, ap.h,
                                z0 === nothing ? C_NULL : pointer(z0), seed), cl.ctx.h)
end
"x_bias <- column mean of x [S*n] (polee_classify.py:75)"
function init_bias!(cl::LogisticRegression, x::Vector{Float32}, S::Integer)
    GC.@preserve x check(ccall((:polee_classify_init_bias_points, LIB), Cint, (Ptr{Cvoid}, Ptr{Float32}, Int32), cl.h, x, S), cl.ctx.h)
end
"loss_sample (polee_classify.py:43-49) and its gradients (loss, g_w [n*k], g_x_bias [n], g_z_bias [k]); no update"
function loss_and_gradients(cl::LogisticRegression, ap::ApproxLikelihood, labels::Vector{Float32}; seed::Integer=0,
                            z0::Union{Nothing,Vector{Float32}}=nothing)
    loss = Ref{Float32}(0)
    gw = Vector{Float32}(undef, cl.n * cl.k); gxb = Vector{Float32}(undef, cl.n); gzb = Vector{Float32}(undef, cl.k)
    GC.@preserve labels z0 gw gxb gzb check(
        ccall((:polee_classify_eval, LIB), Cint,
              (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float32}, Ptr{Float32}, UInt64, Ref{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}),
              cl.h, ap.h, labels, z0 === nothing ? C_NULL : pointer(z0), seed, loss, gw, gxb, gzb), cl.ctx.h)
    return loss[], gw, gxb, gzb
end
"loss (polee_classify.py:22-41) and its gradients on a fixed x [S*n]"
function loss_and_gradients(cl::LogisticRegression, x::Vector{Float32}, S::Integer, labels::Vector{Float32})
    loss = Ref{Float32}(0)
    gw = Vector{Float32}(undef, cl.n * cl.k); gxb = Vector{Float32}(undef, cl.n); gzb = Vector{Float32}(undef, cl.k)
    GC.@preserve x labels gw gxb gzb check(
        ccall((:polee_classify_eval_points, LIB), Cint,
              (Ptr{Cvoid}, Ptr{Float32}, Int32, Ptr{Float32}, Ref{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}),
              cl.h, x, S, labels, loss, gw, gxb, gzb), cl.ctx.h)
    return loss[], gw, gxb, gzb
end
"niter Adam steps on fresh draws (fit_sample, polee_classify.py:57-72; call init_bias! first): the loss trace"
function fit!(cl::LogisticRegression, ap::ApproxLikelihood, labels::Vector{Float32}, niter::Integer; seed::Integer=0,
              z0::Union{Nothing,Vector{Float32}}=nothing)
    trace = Vector{Float32}(undef, niter)
    GC.@preserve labels z0 trace check(
        ccall((:polee_classify_fit, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float32}, Int32, UInt64, Ptr{Float32}, Ptr{Float32}),
              cl.h, ap.h, labels, niter, seed, z0 === nothing ? C_NULL : pointer(z0), trace), cl.ctx.h)
    return trace
end
"fit (polee_classify.py:74-95) on a fixed x [S*n]"
function fit!(cl::LogisticRegression, x::Vector{Float32}, S::Integer, labels::Vector{Float32}, niter::Integer)
    trace = Vector{Float32}(undef, niter)
    GC.@preserve x labels trace check(
        ccall((:polee_classify_fit_points, LIB), Cint, (Ptr{Cvoid}, Ptr{Float32}, Int32, Ptr{Float32}, Int32, Ptr{Float32}),
              cl.h, x, S, labels, niter, trace), cl.ctx.h)
    return trace
end
"predict_sample (polee_classify.py:105-111): probabilities [S*k], the mean over ndraws draws"
function predict(cl::LogisticRegression, ap::ApproxLikelihood, ndraws::Integer; seed::Integer=0,
                 z0::Union{Nothing,Vector{Float32}}=nothing)
    probs = Vector{Float32}(undef, ap.S * cl.k)
    GC.@preserve z0 probs check(
        ccall((:polee_classify_predict, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Int32, UInt64, Ptr{Float32}, Ptr{Float32}),
              cl.h, ap.h, ndraws, seed, z0 === nothing ? C_NULL : pointer(z0), probs), cl.ctx.h)
    return probs
end
"predict (polee_classify.py:113-114)"
function predict(cl::LogisticRegression, x::Vector{Float32}, S::Integer)
    probs = Vector{Float32}(undef, S * cl.k)
    GC.@preserve x probs check(ccall((:polee_classify_predict_points, LIB), Cint, (Ptr{Cvoid}, Ptr{Float32}, Int32, Ptr{Float32}),
                                     cl.h, x, S, probs), cl.ctx.h)
    return probs
end

# ---- `polee model tsne` (models/tsne.jl:52-99, models/polee_tsne.py:213-398): parametric t-SNE on posterior draws ------------------
"mirror of `polee_tsne_opts` (include/polee_hip.h): field order and types must stay in step with the header"
mutable struct TSNEOpts
    num_components::Int32; use_vlr::Int32
    alpha::Float32; eps::Float32; learning_rate::Float32
    beta1::Float32; beta2::Float32; epsilon::Float32
    function TSNEOpts()
        o = new()
        ccall((:polee_tsne_default_opts, LIB), Cvoid, (Ref{TSNEOpts},), o)
        return o
    end
end

"the embedding z = lx W of estimate_tsne (polee_tsne.py:293-298); matrices are row-major vectors: W [n*C] (transcript by transcript),
z [S*C] (sample by sample), delta [S*S]; batches hold 0-based sample indices"
mutable struct TSNE
    h::Ptr{Cvoid}
    ctx::Context
    n::Int
    S::Int
    C::Int
end
function TSNE(ctx::Context, n::Integer, S::Integer; opts::TSNEOpts=TSNEOpts())
    r = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:polee_tsne_create, LIB), Cint, (Ptr{Cvoid}, Int32, Int32, Ref{TSNEOpts}, Ref{Ptr{Cvoid}}), ctx.h, n, S, opts, r), ctx.h)
    ts = TSNE(r[], ctx, n, S, opts.num_components)
    finalizer(x -> ccall((:polee_tsne_destroy, LIB), Cvoid, (Ptr{Cvoid},), x.h), ts)
    return ts
end
function get_params(ts::TSNE)
    w = Vector{Float32}(undef, ts.n * ts.C)
    GC.@preserve w check(ccall((:polee_tsne_get_params, LIB), Cint, (Ptr{Cvoid}, Ptr{Float32}), ts.h, w), ts.ctx.h)
    return w
end
function set_params!(ts::TSNE, w::Vector{Float32})
    GC.@preserve w check(ccall((:polee_tsne_set_params, LIB), Cint, (Ptr{Cvoid}, Ptr{Float32}), ts.h, w), ts.ctx.h)
end
"Adam moments and step clock back to zero"
reset!(ts::TSNE) = check(ccall((:polee_tsne_reset, LIB), Cint, (Ptr{Cvoid},), ts.h), ts.ctx.h)
"the bandwidths of find_sigmas (polee_tsne.py:64-103), [S]"
function set_sigmas!(ts::TSNE, sigmas::Vector{Float32})
    GC.@preserve sigmas check(ccall((:polee_tsne_set_sigmas, LIB), Cint, (Ptr{Cvoid}, Ptr{Float32}), ts.h, sigmas), ts.ctx.h)
end
"delta [S*S] of one draw (pairwise_vlr, polee_tsne.py:17-26)"
function distances(ts::TSNE, ap::ApproxLikelihood; seed::Integer=0, z0::Union{Nothing,Vector{Float32}}=nothing)
    delta = Vector{Float64}(undef, ts.S * ts.S)
    GC.@preserve z0 delta check(
        ccall((:polee_tsne_distances, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Float32}, UInt64, Ptr{Float64}),
              ts.h, ap.h, z0 === nothing ? C_NULL : pointer(z0), seed, delta), ts.ctx.h)
    return delta
end
"delta [S*S] of a fixed x [S*n]"
function distances(ts::TSNE, x::Vector{Float32})
    delta = Vector{Float64}(undef, ts.S * ts.S)
    GC.@preserve x delta check(ccall((:polee_tsne_distances_points, LIB), Cint, (Ptr{Cvoid}, Ptr{Float32}, Ptr{Float64}), ts.h, x, delta),
                               ts.ctx.h)
    return delta
end
"the loss (polee_tsne.py:337) of one evaluation on `batch` and its gradient (loss, g_w [n*C]); no update"
function loss_and_gradient(ts::TSNE, ap::ApproxLikelihood, batch::Vector{Int32}; seed::Integer=0,
                           z0::Union{Nothing,Vector{Float32}}=nothing)
    loss = Ref{Float32}(0)
    gw = Vector{Float32}(undef, ts.n * ts.C)
    GC.@preserve batch z0 gw check(
        ccall((:polee_tsne_eval, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Int32}, Int32, Ptr{Float32}, UInt64, Ref{Float32}, Ptr{Float32}),
              ts.h, ap.h, batch, length(batch), z0 === nothing ? C_NULL : pointer(z0), seed, loss, gw), ts.ctx.h)
    return loss[], gw
end
function loss_and_gradient(ts::TSNE, x::Vector{Float32}, batch::Vector{Int32})
    loss = Ref{Float32}(0)
    gw = Vector{Float32}(undef, ts.n * ts.C)
    GC.@preserve x batch gw check(
        ccall((:polee_tsne_eval_points, LIB), Cint, (Ptr{Cvoid}, Ptr{Float32}, Ptr{Int32}, Int32, Ref{Float32}, Ptr{Float32}),
              ts.h, x, batch, length(batch), loss, gw), ts.ctx.h)
    return loss[], gw
end
"niter Adam steps on fresh draws (polee_tsne.py:355-375), step i on batches[(i-1)*B+1 : i*B]: the loss trace"
function fit!(ts::TSNE, ap::ApproxLikelihood, batches::Vector{Int32}, B::Integer, niter::Integer; seed::Integer=0,
              z0::Union{Nothing,Vector{Float32}}=nothing)
    trace = Vector{Float32}(undef, niter)
    GC.@preserve batches z0 trace check(
        ccall((:polee_tsne_fit, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Int32}, Int32, Int32, UInt64, Ptr{Float32}, Ptr{Float32}),
              ts.h, ap.h, batches, B, niter, seed, z0 === nothing ? C_NULL : pointer(z0), trace), ts.ctx.h)
    return trace
end
function fit!(ts::TSNE, x::Vector{Float32}, batches::Vector{Int32}, B::Integer, niter::Integer)
    trace = Vector{Float32}(undef, niter)
    GC.@preserve x batches trace check(
        ccall((:polee_tsne_fit_points, LIB), Cint, (Ptr{Cvoid}, Ptr{Float32}, Ptr{Int32}, Int32, Int32, Ptr{Float32}),
              ts.h, x, batches, B, niter, trace), ts.ctx.h)
    return trace
end
"the mean of z over ndraws draws (polee_tsne.py:392-395), [S*C]"
function embed(ts::TSNE, ap::ApproxLikelihood, ndraws::Integer; seed::Integer=0, z0::Union{Nothing,Vector{Float32}}=nothing)
    z = Vector{Float32}(undef, ts.S * ts.C)
    GC.@preserve z0 z check(
        ccall((:polee_tsne_embed, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Int32, UInt64, Ptr{Float32}, Ptr{Float32}),
              ts.h, ap.h, ndraws, seed, z0 === nothing ? C_NULL : pointer(z0), z), ts.ctx.h)
    return z
end
function embed(ts::TSNE, x::Vector{Float32})
    z = Vector{Float32}(undef, ts.S * ts.C)
    GC.@preserve x z check(ccall((:polee_tsne_embed_points, LIB), Cint, (Ptr{Cvoid}, Ptr{Float32}, Ptr{Float32}), ts.h, x, z), ts.ctx.h)
    return z
end

# ---- `polee model random-forest` (models/random-forest.jl; csrc/forest.hip, csrc/forest_host.cpp): forests on posterior draws -------
"mirror of `polee_forest_opts` (include/polee_hip.h): field order and types must stay in step with the header"
mutable struct ForestOpts
    ntrees::Int32; max_depth::Int32; min_samples_leaf::Int32; min_samples_split::Int32
    nsubfeatures::Float64; partial_sampling::Float64
    function ForestOpts()
        o = new()
        ccall((:polee_forest_default_opts, LIB), Cvoid, (Ref{ForestOpts},), o)
        return o
    end
end

"the node arrays of a forest: tree t owns nodes tree_off[t]+1 : tree_off[t+1] (0-based offsets, 0-based node numbers within a tree)"
struct ForestNodes
    tree_off::Vector{Int64}
    feature::Vector{Int32}
    threshold::Vector{Float64}
    left::Vector{Int32}
    right::Vector{Int32}
    label::Vector{Int32}
end

"a forest of k classes on n features; x matrices are row-major vectors [rows*n], labels 0-based class numbers"
mutable struct Forest
    h::Ptr{Cvoid}
    ctx::Context
    n::Int
    k::Int
end
function Forest(ctx::Context, n::Integer, k::Integer; opts::ForestOpts=ForestOpts())
    r = Ref{Ptr{Cvoid}}(C_NULL)
    check(ccall((:polee_forest_create, LIB), Cint, (Ptr{Cvoid}, Int32, Int32, Ref{ForestOpts}, Ref{Ptr{Cvoid}}), ctx.h, n, k, opts, r), ctx.h)
    f = Forest(r[], ctx, n, k)
    finalizer(x -> ccall((:polee_forest_destroy, LIB), Cvoid, (Ptr{Cvoid},), x.h), f)
    return f
end
function fit!(f::Forest, x::Vector{Float32}, labels::Vector{Int32}; seed::Integer=12346)
    GC.@preserve x labels check(
        ccall((:polee_forest_fit_points, LIB), Cint, (Ptr{Cvoid}, Ptr{Float32}, Ptr{Int32}, Int32, UInt64), f.h, x, labels, length(labels), seed),
        f.ctx.h)
    return f
end
"trains on ndraws draws of every sample of `ap` (row d*S + s carries labels[s])"
function fit!(f::Forest, ap::ApproxLikelihood, labels::Vector{Int32}, ndraws::Integer; draw_seed::Integer=12345, seed::Integer=12346,
              z0::Union{Nothing,Vector{Float32}}=nothing)
    GC.@preserve labels z0 check(
        ccall((:polee_forest_fit, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Int32}, Int32, UInt64, UInt64, Ptr{Float32}),
              f.h, ap.h, labels, ndraws, draw_seed, seed, z0 === nothing ? C_NULL : pointer(z0)), f.ctx.h)
    return f
end
function nodes(f::Forest)
    nt = Ref{Int32}(0)
    nn = Ref{Int64}(0)
    check(ccall((:polee_forest_node_count, LIB), Cint, (Ptr{Cvoid}, Ref{Int32}, Ref{Int64}), f.h, nt, nn), f.ctx.h)
    fo = ForestNodes(Vector{Int64}(undef, nt[] + 1), Vector{Int32}(undef, nn[]), Vector{Float64}(undef, nn[]), Vector{Int32}(undef, nn[]),
                     Vector{Int32}(undef, nn[]), Vector{Int32}(undef, nn[]))
    check(ccall((:polee_forest_get_nodes, LIB), Cint,
                (Ptr{Cvoid}, Ptr{Int64}, Ptr{Int32}, Ptr{Float64}, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}),
                f.h, fo.tree_off, fo.feature, fo.threshold, fo.left, fo.right, fo.label), f.ctx.h)
    return fo
end
function set_nodes!(f::Forest, fo::ForestNodes)
    check(ccall((:polee_forest_set_nodes, LIB), Cint,
                (Ptr{Cvoid}, Int32, Ptr{Int64}, Ptr{Int32}, Ptr{Float64}, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}),
                f.h, length(fo.tree_off) - 1, fo.tree_off, fo.feature, fo.threshold, fo.left, fo.right, fo.label), f.ctx.h)
end
"votes [R*k] of the forest on x [R*n]"
function votes(f::Forest, x::Vector{Float32})
    R = div(length(x), f.n)
    v = Vector{Int32}(undef, R * f.k)
    GC.@preserve x v check(ccall((:polee_forest_predict_points, LIB), Cint, (Ptr{Cvoid}, Ptr{Float32}, Int32, Ptr{Int32}), f.h, x, R, v), f.ctx.h)
    return v
end
"votes [S*k] summed over ndraws draws of every sample of `ap`"
function votes(f::Forest, ap::ApproxLikelihood, ndraws::Integer; seed::Integer=12347, z0::Union{Nothing,Vector{Float32}}=nothing)
    v = Vector{Int32}(undef, ap.S * f.k)
    GC.@preserve z0 v check(
        ccall((:polee_forest_predict, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Int32, UInt64, Ptr{Float32}, Ptr{Int32}),
              f.h, ap.h, ndraws, seed, z0 === nothing ? C_NULL : pointer(z0), v), f.ctx.h)
    return v
end
"the rows [ndraws*S*n] training and prediction see: the device's logf of the draws"
function forest_log_draws(ap::ApproxLikelihood, ndraws::Integer; seed::Integer=12345, z0::Union{Nothing,Vector{Float32}}=nothing)
    out = Vector{Float32}(undef, ndraws * ap.S * ap.n)
    GC.@preserve z0 out check(
        ccall((:polee_forest_log_draws, LIB), Cint, (Ptr{Cvoid}, Int32, UInt64, Ptr{Float32}, Ptr{Float32}),
              ap.h, ndraws, seed, z0 === nothing ? C_NULL : pointer(z0), out))
    return out
end
"the same forest on the host, no context"
function forest_build_host(x::Vector{Float32}, labels::Vector{Int32}, n::Integer, k::Integer; opts::ForestOpts=ForestOpts(),
                           seed::Integer=12346)
    N = length(labels)
    nn = Ref{Int64}(0)
    GC.@preserve x labels check(
        ccall((:polee_forest_build_host, LIB), Cint,
              (Ptr{Float32}, Ptr{Int32}, Int32, Int32, Int32, Ref{ForestOpts}, UInt64, Int64, Ref{Int64}, Ptr{Int64}, Ptr{Int32},
               Ptr{Float64}, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}),
              x, labels, N, n, k, opts, seed, 0, nn, C_NULL, C_NULL, C_NULL, C_NULL, C_NULL, C_NULL))
    c = nn[]
    fo = ForestNodes(Vector{Int64}(undef, opts.ntrees + 1), Vector{Int32}(undef, c), Vector{Float64}(undef, c), Vector{Int32}(undef, c),
                     Vector{Int32}(undef, c), Vector{Int32}(undef, c))
    GC.@preserve x labels check(
        ccall((:polee_forest_build_host, LIB), Cint,
              (Ptr{Float32}, Ptr{Int32}, Int32, Int32, Int32, Ref{ForestOpts}, UInt64, Int64, Ref{Int64}, Ptr{Int64}, Ptr{Int32},
               Ptr{Float64}, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}),
              x, labels, N, n, k, opts, seed, c, nn, fo.tree_off, fo.feature, fo.threshold, fo.left, fo.right, fo.label))
    return fo
end
function forest_votes_host(fo::ForestNodes, x::Vector{Float32}, n::Integer, k::Integer)
    R = div(length(x), n)
    v = Vector{Int32}(undef, R * k)
    GC.@preserve x v check(
        ccall((:polee_forest_votes_host, LIB), Cint,
              (Int32, Int32, Int32, Ptr{Int64}, Ptr{Int32}, Ptr{Float64}, Ptr{Int32}, Ptr{Int32}, Ptr{Int32}, Ptr{Float32}, Int32, Ptr{Int32}),
              n, k, length(fo.tree_off) - 1, fo.tree_off, fo.feature, fo.threshold, fo.left, fo.right, fo.label, x, R, v))
    return v
end

# ---- isoform effect sizes (estimate_isoform_effect_sizes, src/regression.jl:761-945; csrc/effects.hip) -----------------------------
"the transcripts of `gene_of` (0-based gene of every transcript, any order) segmented by gene once, on creation"
mutable struct IsoformEffects
    h::Ptr{Cvoid}
    ctx::Context
    n::Int
    G::Int
    F::Int
end
function IsoformEffects(ctx::Context, gene_of::Vector{Int32}, G::Integer, F::Integer)
    r = Ref{Ptr{Cvoid}}(C_NULL)
    GC.@preserve gene_of check(ccall((:polee_effects_create, LIB), Cint, (Ptr{Cvoid}, Int32, Int32, Ptr{Int32}, Int32, Ref{Ptr{Cvoid}}),
                                     ctx.h, length(gene_of), G, gene_of, F, r), ctx.h)
    fx = IsoformEffects(r[], ctx, length(gene_of), G, F)
    finalizer(x -> ccall((:polee_effects_destroy, LIB), Cvoid, (Ptr{Cvoid},), x.h), fx)
    return fx
end
"(min_effect_sizes, mean_effect_sizes, prob_de [F*n], aitchison_min, aitchison_mean, aitchison_prob_de [F*G], kernel ms), row-major
vectors; a threshold of `nothing` leaves its prob_de at zero; prob_de is one-sided, #{e > effect_size} / niter (:850); zx [niter*n]
and zw [niter*F*n] replace the device's noise"
function estimate_isoform_effect_sizes(fx::IsoformEffects, qw_loc::Vector{Float32}, qw_scale::Vector{Float32},
                                       qx_bias_loc::Vector{Float32}, qx_bias_scale::Vector{Float32}; niter::Integer=1000,
                                       target_coverage::Real=0.1, effect_size::Union{Nothing,Real}=nothing,
                                       aitchison_effect_size::Union{Nothing,Real}=nothing, seed::Integer=0,
                                       zx::Union{Nothing,Vector{Float32}}=nothing, zw::Union{Nothing,Vector{Float32}}=nothing)
    mn = Vector{Float32}(undef, fx.F * fx.n); me = similar(mn); pr = similar(mn)
    amn = Vector{Float32}(undef, fx.F * fx.G); ame = similar(amn); apr = similar(amn)
    ms = Ref{Float64}(0)
    GC.@preserve qw_loc qw_scale qx_bias_loc qx_bias_scale zx zw mn me pr amn ame apr check(
        ccall((:polee_effects_run, LIB), Cint,
              (Ptr{Cvoid}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Int32, Float64, Float64, Float64, UInt64,
               Ptr{Float32}, Int64, Ptr{Float32}, Int64, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32},
               Ptr{Float32}, Ref{Float64}),
              fx.h, qw_loc, qw_scale, qx_bias_loc, qx_bias_scale, niter, target_coverage,
              effect_size === nothing ? NaN : Float64(effect_size), aitchison_effect_size === nothing ? NaN : Float64(aitchison_effect_size),
              seed, zx === nothing ? C_NULL : pointer(zx), zx === nothing ? 0 : length(zx), zw === nothing ? C_NULL : pointer(zw),
              zw === nothing ? 0 : length(zw), mn, me, pr, amn, ame, apr, ms), fx.ctx.h)
    return mn, me, pr, amn, ame, apr, ms[]
end

# ---- the alternative approximations (src/likelihood-approximation-alt.jl; `prep --approx-method`) ---------------------------------
const ALT_LOGISTIC_NORMAL, ALT_KUMARASWAMY_PTT, ALT_LOGIT_NORMAL_PTT, ALT_NORMAL_ILR, ALT_NORMAL_ALR = Int32(1), Int32(2), Int32(3), Int32(4), Int32(5)

"mirror of `polee_altvi_opts` (include/polee_hip.h): field order and types must stay in step with the header"
mutable struct AltViOpts
    method::Int32; num_steps::Int32; num_mc_samples::Int32; gradonly::Int32; refidx::Int32; reserved::Int32
    seed::UInt64; z0::Ptr{Float32}; eps::Float64
    adam_initial_learning_rate::Float64; adam_learning_rate_decay::Float64; adam_min_learning_rate::Float64
    adam_eps::Float64; adam_rv::Float64; adam_rm::Float64
    max_step0::Float64; max_step1::Float64
    AltViOpts(method::Integer) = (o = new(); ccall((:polee_altvi_default_opts, LIB), Cvoid, (Int32, Ref{AltViOpts}), method, o); o)
end
mutable struct AltViStats
    steps_done::Int32
    nonfinite_step::Int32
    last_elbo::Float64
    last_lp_mean::Float64
    AltViStats() = new(0, 0, 0.0, 0.0)
end

"State of one fit of approximate_likelihood(::LogisticNormalApprox | ::NormalILRApprox | ::NormalALRApprox, sample); t: the tree of normal_ilr"
mutable struct AltLikelihoodApproximationFit
    h::Ptr{Cvoid}
    sample::AnySample
    t::Union{Nothing,PolyaTreeTransform}
    K::Int
    function AltLikelihoodApproximationFit(s::AnySample, opts::AltViOpts, t::Union{Nothing,PolyaTreeTransform}=nothing)
        out = Ref{Ptr{Cvoid}}(C_NULL)
        check(ccall((:polee_altvi_create, LIB), Cint, (Ptr{Cvoid}, Ptr{Cvoid}, Ref{AltViOpts}, Ref{Ptr{Cvoid}}),
                    s.h, t === nothing ? C_NULL : t.h, opts, out), s.ctx.h)
        f = new(out[], s, t, Int(opts.num_mc_samples))
        finalizer(x -> ccall((:polee_altvi_destroy, LIB), Cvoid, (Ptr{Cvoid},), x.h), f)
        return f
    end
end
run!(f::AltLikelihoodApproximationFit, nsteps::Integer) =
    check(ccall((:polee_altvi_run, LIB), Cint, (Ptr{Cvoid}, Int32), f.h, nsteps), f.sample.ctx.h)
sync!(f::AltLikelihoodApproximationFit) = check(ccall((:polee_altvi_sync, LIB), Cint, (Ptr{Cvoid},), f.h), f.sample.ctx.h)
function params(f::AltLikelihoodApproximationFit)
    mu, omega = (Vector{Float32}(undef, f.sample.n - 1) for _ in 1:2)
    GC.@preserve mu omega check(ccall((:polee_altvi_get_params, LIB), Cint, (Ptr{Cvoid}, Ptr{Float32}, Ptr{Float32}), f.h, mu, omega),
                                f.sample.ctx.h)
    return mu, omega
end
function set_params!(f::AltLikelihoodApproximationFit, mu::Vector{Float32}, omega::Vector{Float32})
    GC.@preserve mu omega check(ccall((:polee_altvi_set_params, LIB), Cint, (Ptr{Cvoid}, Ptr{Float32}, Ptr{Float32}), f.h, mu, omega),
                                f.sample.ctx.h)
end
function stats(f::AltLikelihoodApproximationFit)
    st = AltViStats()
    check(ccall((:polee_altvi_get_stats, LIB), Cint, (Ptr{Cvoid}, Ref{AltViStats}), f.h, st), f.sample.ctx.h)
    return st
end
"per-step elbo and mean log-likelihood (gradonly == 0 only)"
function trace(f::AltLikelihoodApproximationFit)
    k = Int(stats(f).steps_done)
    elbo, lp = Vector{Float64}(undef, k), Vector{Float64}(undef, k)
    GC.@preserve elbo lp check(ccall((:polee_altvi_get_trace, LIB), Cint, (Ptr{Cvoid}, Ptr{Float64}, Ptr{Float64}), f.h, elbo, lp),
                               f.sample.ctx.h)
    return elbo, lp
end
"the N(0,1) draws of iteration `step`: Float32 [n-1, K]"
function export_noise(f::AltLikelihoodApproximationFit, step::Integer)
    z = Matrix{Float32}(undef, f.sample.n - 1, f.K)
    GC.@preserve z check(ccall((:polee_altvi_export_noise, LIB), Cint, (Ptr{Cvoid}, Int32, Ptr{Float32}), f.h, step, z), f.sample.ctx.h)
    return z
end
"test hook: the next step's draws and averaged gradients at the current parameters, nothing updated"
function eval_gradients(f::AltLikelihoodApproximationFit)
    n, K = f.sample.n, f.K
    xs = Matrix{Float32}(undef, n, K); xg = Matrix{Float64}(undef, n, K); yg = Matrix{Float64}(undef, n - 1, K)
    mg, og = (Vector{Float32}(undef, n - 1) for _ in 1:2)
    lp, ladj = Vector{Float64}(undef, K), Vector{Float64}(undef, K)
    GC.@preserve xs xg yg mg og lp ladj check(
        ccall((:polee_altvi_eval_gradients, LIB), Cint,
              (Ptr{Cvoid}, Ptr{Float32}, Ptr{Float64}, Ptr{Float64}, Ptr{Float32}, Ptr{Float32}, Ptr{Float64}, Ptr{Float64}),
              f.h, xs, xg, yg, mg, og, lp, ladj), f.sample.ctx.h)
    return xs, xg, yg, mg, og, lp, ladj
end
"sample_likap (src/evaluate.jl:34-74, 203-275): Float32 [n, count], every draw divided by the effective lengths and renormalised"
function alt_sample(ctx::Context, method::Integer, t::Union{Nothing,PolyaTreeTransform}, mu::Vector{Float32}, omega::Vector{Float32},
                    efflens::Vector{Float32}, refidx::Integer, count::Integer; seed::Integer=123456789,
                    z0::Union{Nothing,Matrix{Float32}}=nothing)
    n = length(efflens)
    out = Matrix{Float32}(undef, n, count)
    GC.@preserve mu omega efflens z0 out check(
        ccall((:polee_alt_sample, LIB), Cint,
              (Ptr{Cvoid}, Int32, Ptr{Cvoid}, Int32, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Int32, Int32, UInt64, Ptr{Float32}, Ptr{Float32}),
              ctx.h, method, t === nothing ? C_NULL : t.h, n, mu, omega, efflens, refidx, count, seed,
              z0 === nothing ? C_NULL : pointer(z0), out), ctx.h)
    return out
end
"a, b of the ILR balances for r, s leaves below the left and right child (isometric_log_ratios.jl:62-66): Float64 [2, count]"
function ilr_coefficients(r::Vector{Int32}, s::Vector{Int32})
    ab = Matrix{Float64}(undef, 2, length(r))
    GC.@preserve r s ab check(ccall((:polee_ilr_coefficients, LIB), Cint, (Ptr{Int32}, Ptr{Int32}, Int64, Ptr{Float64}), r, s, length(r), ab))
    return ab
end

# ---- training of the fragment bias model (src/bias.jl; csrc/bias_train.hip, csrc/bias_train_host.cpp): BiasModel(...) from fragments -------
"mirror of `polee_bias_train_opts` (include/polee_hip.h): field order and types must stay in step with the header"
struct BiasTrainOpts
    seed::UInt64
    host::Int32
    reserved::Int32
end
"a trainer with its examples made; ctx === nothing runs the host trainer (POLEE_HOST_THREADS)"
mutable struct BiasTrainer
    h::Ptr{Cvoid}
    ctx::Union{Nothing,Context}
end
_bt_ctx(ctx::Union{Nothing,Context}) = ctx === nothing ? C_NULL : ctx.h
function _bt_finish(r::Ref{Ptr{Cvoid}}, ctx)
    bt = BiasTrainer(r[], ctx)
    finalizer(x -> ccall((:polee_bias_train_destroy, LIB), Cvoid, (Ptr{Cvoid},), x.h), bt)
    return bt
end
"""
examples from fragments (BiasTrainingExample, bias.jl:21-80): tseq_ptr [n+1] 0-based offsets, tseq codes 0 A 1 C 2 G 3 T 4 other;
fragments (transcript 0-based, tpos 1-based, fraglen); background === nothing draws one background fragment per foreground fragment
"""
function BiasTrainer(ctx::Union{Nothing,Context}, tseq_ptr::Vector{Int64}, tseq::Vector{UInt8}, transcript::Vector{Int32},
                     tpos::Vector{Int64}, fraglen::Vector{Int32};
                     background::Union{Nothing,Tuple{Vector{Int32},Vector{Int64},Vector{Int32}}}=nothing, seed::Integer=0)
    r = Ref{Ptr{Cvoid}}(C_NULL)
    opts = Ref(BiasTrainOpts(seed, ctx === nothing ? 1 : 0, 0))
    bt_, bp_, bf_ = background === nothing ? (Int32[], Int64[], Int32[]) : background
    GC.@preserve tseq_ptr tseq transcript tpos fraglen bt_ bp_ bf_ check(
        ccall((:polee_bias_train_create, LIB), Cint,
              (Ptr{Cvoid}, Int32, Ptr{Int64}, Ptr{UInt8}, Int64, Ptr{Int32}, Ptr{Int64}, Ptr{Int32}, Int64, Ptr{Int32}, Ptr{Int64}, Ptr{Int32},
               Ref{BiasTrainOpts}, Ref{Ptr{Cvoid}}),
              _bt_ctx(ctx), length(tseq_ptr) - 1, tseq_ptr, tseq, length(transcript), transcript, tpos, fraglen, length(bt_),
              background === nothing ? C_NULL : pointer(bt_), background === nothing ? C_NULL : pointer(bp_),
              background === nothing ? C_NULL : pointer(bf_), opts, r), _bt_ctx(ctx))
    return _bt_finish(r, ctx)
end
"ready-made examples (--dump-bias-training-examples): left / right UInt8 [20, N] codes (column = example), frag_gc [N], the first n_fg foreground"
function BiasTrainer(ctx::Union{Nothing,Context}, left::Matrix{UInt8}, right::Matrix{UInt8}, frag_gc::Vector{Float64}, n_fg::Integer;
                     seed::Integer=0)
    r = Ref{Ptr{Cvoid}}(C_NULL)
    opts = Ref(BiasTrainOpts(seed, ctx === nothing ? 1 : 0, 0))
    GC.@preserve left right frag_gc check(
        ccall((:polee_bias_train_create_from_examples, LIB), Cint,
              (Ptr{Cvoid}, Int64, Int64, Ptr{UInt8}, Ptr{UInt8}, Ptr{Float64}, Ref{BiasTrainOpts}, Ref{Ptr{Cvoid}}),
              _bt_ctx(ctx), n_fg, length(frag_gc) - n_fg, left, right, frag_gc, opts, r), _bt_ctx(ctx))
    return _bt_finish(r, ctx)
end
"BiasModel(...) (bias.jl:677-785)"
function train!(bt::BiasTrainer)
    check(ccall((:polee_bias_train_run, LIB), Cint, (Ptr{Cvoid},), bt.h), _bt_ctx(bt.ctx))
    return bt
end
"orders [20] x 2, ps Float32 [4096, 4, 20] x 2 (column-major view of the C [20][4][4096]), gc_bins [100], gc_qs [14], accuracy (a fraction)"
function bias_model(bt::BiasTrainer)
    ol, or_ = Vector{Int32}(undef, 20), Vector{Int32}(undef, 20)
    pl, pr = Array{Float32}(undef, 4096, 4, 20), Array{Float32}(undef, 4096, 4, 20)
    bins, qs, acc = Vector{Float32}(undef, 100), Vector{Float32}(undef, 14), Ref{Float64}(0)
    GC.@preserve ol or_ pl pr bins qs check(
        ccall((:polee_bias_train_get_model, LIB), Cint,
              (Ptr{Cvoid}, Ptr{Int32}, Ptr{Int32}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ptr{Float32}, Ref{Float64}),
              bt.h, ol, or_, pl, pr, bins, qs, acc), _bt_ctx(bt.ctx))
    return (orders_left=ol, orders_right=or_, ps_left=pl, ps_right=pr, gc_bins=bins, gc_qs=qs, accuracy=acc[])
end
"the packed examples: left / right UInt64 [N] (20 two-bit codes, position 1 highest), frag_gc [N], bg_tpos [n_bg] (positions: from fragments only)"
function bias_examples(bt::BiasTrainer; positions::Bool=true)
    nf, nb = Ref{Int64}(0), Ref{Int64}(0)
    check(ccall((:polee_bias_train_get_examples, LIB), Cint,
                (Ptr{Cvoid}, Ref{Int64}, Ref{Int64}, Ptr{UInt64}, Ptr{UInt64}, Ptr{Float64}, Ptr{Int64}),
                bt.h, nf, nb, C_NULL, C_NULL, C_NULL, C_NULL), _bt_ctx(bt.ctx))
    N = nf[] + nb[]
    l, r, g, bp = Vector{UInt64}(undef, N), Vector{UInt64}(undef, N), Vector{Float64}(undef, N), Vector{Int64}(undef, positions ? nb[] : 0)
    GC.@preserve l r g bp check(
        ccall((:polee_bias_train_get_examples, LIB), Cint,
              (Ptr{Cvoid}, Ptr{Int64}, Ptr{Int64}, Ptr{UInt64}, Ptr{UInt64}, Ptr{Float64}, Ptr{Int64}),
              bt.h, C_NULL, C_NULL, l, r, g, positions ? pointer(bp) : C_NULL), _bt_ctx(bt.ctx))
    return (n_fg=nf[], n_bg=nb[], left=l, right=r, frag_gc=g, bg_tpos=bp)
end
"the search of one side (0 left, 1 right): positions (0-based) of the committed rounds, losses [rounds + 1]"
function bias_trace(bt::BiasTrainer, side::Integer)
    rounds, pos, loss = Ref{Int32}(0), Vector{Int32}(undef, 140), Vector{Float64}(undef, 141)
    GC.@preserve pos loss check(
        ccall((:polee_bias_train_get_trace, LIB), Cint, (Ptr{Cvoid}, Int32, Ref{Int32}, Ptr{Int32}, Ptr{Float64}), bt.h, side, rounds, pos, loss),
        _bt_ctx(bt.ctx))
    return pos[1:rounds[]], loss[1:rounds[]+1]
end
"debug: the 20 candidate losses of ONE round from the state `orders` (-1 .. 6) and the loss of that state"
function bias_candidates(bt::BiasTrainer, side::Integer, orders::Vector{Int32})
    losses, loss0 = Vector{Float64}(undef, 20), Ref{Float64}(0)
    GC.@preserve orders losses check(
        ccall((:polee_bias_train_candidates, LIB), Cint, (Ptr{Cvoid}, Int32, Ptr{Int32}, Ptr{Float64}, Ref{Float64}), bt.h, side, orders, losses, loss0),
        _bt_ctx(bt.ctx))
    return losses, loss0[]
end

const SPLICE_TYPE_NAMES = ["cassette_exon", "mutex_exon", "alt_acceptor_site", "alt_donor_site", "retained_intron", "alt_5p_end", "alt_3p_end"]
"""
    splicing_features(T; gene_of=nothing, ctx=nothing)

splicing_features (src/splicing.jl:98-230) from the exon structure (polee_splice_run; ctx = nothing: polee_splice_run_host, the same
arrays from the host threads).  T: NamedTuple (seq, strand, exon_ptr, exon_first, exon_last) in the layout of polee_xb_transcripts;
gene_of: Int32 [n], 1-based, for the alternative ends (alt_ends = true).  Returns (num_features, type (0-based index into
SPLICE_TYPE_NAMES), seq, strand, coords Int64 [4, F], end_span Int64 [2, F], included_ptr, included_idx, excluded_ptr, excluded_idx,
feature_idxs, feature_transcript_idxs, antifeature_idxs, antifeature_transcript_idxs); the order is this project's own (DESIGN.md 3.19).
"""
function splicing_features(T; gene_of::Union{Nothing,Vector{Int32}}=nothing, ctx::Union{Nothing,Context}=nothing)
    n = Int32(length(T.seq))
    out = Ref{Ptr{Cvoid}}(C_NULL)
    ch = ctx === nothing ? C_NULL : ctx.h
    g = gene_of === nothing ? Int32[] : gene_of
    GC.@preserve T g begin
        ts = XbTranscripts(n, pointer(T.seq), pointer(T.strand), pointer(T.exon_ptr), pointer(T.exon_first), pointer(T.exon_last))
        gp = gene_of === nothing ? Ptr{Int32}(C_NULL) : pointer(g)
        if ctx === nothing
            check(ccall((:polee_splice_run_host, LIB), Cint, (Ref{XbTranscripts}, Ptr{Int32}, Ref{Ptr{Cvoid}}), ts, gp, out))
        else
            check(ccall((:polee_splice_run, LIB), Cint, (Ptr{Cvoid}, Ref{XbTranscripts}, Ptr{Int32}, Ref{Ptr{Cvoid}}), ch, ts, gp, out), ch)
        end
    end
    h = out[]
    try
        F, ni, ne = Ref{Int64}(0), Ref{Int64}(0), Ref{Int64}(0)
        check(ccall((:polee_splice_sizes, LIB), Cint, (Ptr{Cvoid}, Ref{Int64}, Ref{Int64}, Ref{Int64}, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}),
                    h, F, ni, ne, C_NULL, C_NULL, C_NULL))
        typ, seq, strand = Vector{Int32}(undef, F[]), Vector{Int32}(undef, F[]), Vector{Int8}(undef, F[])
        coords, span = Matrix{Int64}(undef, 4, F[]), Matrix{Int64}(undef, 2, F[])
        iptr, eptr = Vector{Int64}(undef, F[] + 1), Vector{Int64}(undef, F[] + 1)
        iidx, eidx = Vector{Int32}(undef, ni[]), Vector{Int32}(undef, ne[])
        GC.@preserve typ seq strand coords span iptr eptr iidx eidx check(
            ccall((:polee_splice_get, LIB), Cint,
                  (Ptr{Cvoid}, Ptr{Int32}, Ptr{Int32}, Ptr{Int8}, Ptr{Int64}, Ptr{Int64}, Ptr{Int64}, Ptr{Int32}, Ptr{Int64}, Ptr{Int32}),
                  h, typ, seq, strand, coords, span, iptr, iidx, eptr, eidx))
        fidx = Int32[f for f in 1:F[] for _ in iptr[f]+1:iptr[f+1]]
        aidx = Int32[f for f in 1:F[] for _ in eptr[f]+1:eptr[f+1]]
        return (num_features=F[], type=typ, seq=seq, strand=strand, coords=coords, end_span=span, included_ptr=iptr, included_idx=iidx,
                excluded_ptr=eptr, excluded_idx=eidx, feature_idxs=fidx, feature_transcript_idxs=iidx, antifeature_idxs=aidx,
                antifeature_transcript_idxs=eidx)
    finally
        ccall((:polee_splice_destroy, LIB), Cvoid, (Ptr{Cvoid},), h)
    end
end

end # module
