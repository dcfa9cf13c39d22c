# RayuelaHIP.jl -- drop-in bodies for Rayuela.jl's PQ/OPQ encode and ADC linear scan on MI355X.
#
# Host code stays Julia; every body is a `ccall` into librayuela_hip.so (include/rayuela_hip.h).
# Signatures, defaults, return types and index bases are those of the reference:
#   quantize_pq   src/PQ.jl:18-48        quantize_opq  src/OPQ.jl:19-27
#   linscan_pq    src/Linscan.jl:5-37    linscan_opq   src/Linscan.jl:93-115
#   linscan_lsq   src/Linscan.jl:118-157 linscan_cq    src/Linscan.jl:160-193   (SURVEY 8f rank 2)
#   quantize_rvq  src/RVQ.jl:18-66                                              (SURVEY 8f rank 3)
#   quantize_ervq src/ERVQ.jl:19-26      train_ervq    src/ERVQ.jl:51-148
# Julia's column-major arrays are passed as they are: a d-by-n Matrix{Float32} is the C array
# [n][d] the library expects, an m-by-n Matrix{UInt8} is [n][m], k-by-nq outputs are [nq][k].
#
# NOTE: this image has no Julia toolchain, so this file has not been executed here; the identical
# C ABI is exercised through ctypes by tests/ (rayuela.jl_amd/*.py mirrors this file line by line).
module RayuelaHIP

# only quantize_rvq's singleton re-pick needs them (both are Rayuela.jl dependencies, Manifest.toml:79-83,135-139)
import Clustering, Distances

export quantize_pq, quantize_opq, quantize_rvq, linscan_pq, linscan_opq, linscan_lsq, linscan_cq, train_pq, train_opq, train_rvq
export quantize_ervq, train_ervq
export quantize_competitiveq
export get_norms_codebook, quantize_norms
export groundtruth
export encoding_icm, encode_icm_cuda, update_codebooks, update_codebooks_fast_bin, train_lsq, train_lsq_cuda
export train_sr, train_sr_cuda, SR_C_perturb, SR_D_perturb
export quantize_chainq, train_chainq, update_codebooks_chain_bin, get_cbdims_chain
export HipIndex, HipIndexU16, HipAqIndex, HipAqIndexU16, set_codes!, set_codes_synth!, search, HipDataset, quantize
export HipIvfIndex, build!, add!, add_codes!, train_ivfpq
export rerank, search_refine

# Multi-GPU without touching a call site: with ENV["RAYUELA_HIP_DEVICES"] = "0,1,2,3" (or "all") set before the
# call, linscan_pq / linscan_opq below shard B row-wise over those devices inside the library (per-device scan,
# RCCL gather of the per-shard top-k keys, merge on the first device) and quantize_pq / quantize_opq split X over
# them (one PCIe link each).  The results are bit-identical to the single-GPU ones.

# deps/build.jl:64-67 writes the library paths into deps/deps.jl; here one constant / env var.
const librayuela_hip = get(ENV, "RAYUELA_HIP_LIB",
                           joinpath(@__DIR__, "..", "rayuela.jl_amd", "librayuela_hip.so"))

function _check(status::Cint)
  if status != 0
    msg = unsafe_string(ccall((:rq_last_error, librayuela_hip), Cstring, ()))
    error("librayuela_hip status $status: $msg")
  end
  nothing
end

# Result arrays of the scans (the reference's `zeros(Cfloat, k, nq)`, src/Linscan.jl:16-17): every element is written
# by the library, and large ones come page-locked from the library's pool (rq_host_alloc) -- the copy back into a fresh
# pageable array runs at the speed of its first-touch page faults (4.4 ms for the 80 MB of a SIFT1M-shape answer).
# They are ordinary `Matrix{T}` to the caller; the finalizer hands the buffer back when the array is collected.
function _result(::Type{T}, k::Int, nq::Int) where T
  bytes = sizeof(T) * k * nq
  if bytes >= (4 << 20)
    p = ccall((:rq_host_alloc, librayuela_hip), Ptr{Cvoid}, (Csize_t,), bytes)
    if p != C_NULL
      A = unsafe_wrap(Array, Ptr{T}(p), (k, nq); own=false)
      finalizer(a -> ccall((:rq_host_free, librayuela_hip), Cvoid, (Ptr{Cvoid},), pointer(a)), A)
      return A
    end
  end
  return Matrix{T}(undef, k, nq)
end

# cat(C..., dims=3) for even splits; plain concatenation of the column-major blocks otherwise
_cat_codebooks(C::Vector{Matrix{Float32}}) = vcat([vec(Ci) for Ci in C]...)

"""
    quantize_pq(X, C, V=false) -> B     (src/PQ.jl:18-48)
`B::Matrix{Int16}`, m-by-n, one-based.
"""
function quantize_pq(X::Matrix{Float32}, C::Vector{Matrix{Float32}}, V::Bool=false)
  d, n = size(X)
  m    = length(C)
  h    = size(C[1], 2)
  B    = _result(Int16, m, n)
  if V print("Encoding on $m codebooks with librayuela_hip... ") end
  if h > 256      # more than 256 codewords per codebook: 16-bit codes all the way (src/PQ.jl:45-47), rq_encode_pq_wide
    code_base = 1
    _check(ccall((:rq_encode_pq_wide, librayuela_hip), Cint,
      (Ptr{Int16}, Ptr{Cfloat}, Ptr{Cfloat}, Int64, Cint, Cint, Cint, Cint),
      B, X, _cat_codebooks(C), Int64(n), Cint(d), Cint(m), Cint(h), Cint(code_base)))
    if V println("done") end
    return B
  end
  _check(ccall((:rq_encode_pq_i16, librayuela_hip), Cint,
    (Ptr{Int16}, Ptr{Cfloat}, Ptr{Cfloat}, Int64, Cint, Cint, Cint),
    B, X, _cat_codebooks(C), Int64(n), Cint(d), Cint(m), Cint(h)))
  if V println("done") end
  return B
end

"""
    quantize_opq(X, R, C, V=false) -> B     (src/OPQ.jl:19-27) == quantize_pq(R' * X, C, V)
"""
function quantize_opq(X::Matrix{Float32}, R::Matrix{Float32}, C::Vector{Matrix{Float32}}, V::Bool=false)
  d, n = size(X)
  m    = length(C)
  h    = size(C[1], 2)
  B    = _result(Int16, m, n)
  if h > 256      # rq_encode_opq_wide: up to 32767 codewords per codebook
    code_base = 1
    _check(ccall((:rq_encode_opq_wide, librayuela_hip), Cint,
      (Ptr{Int16}, Ptr{Cfloat}, Ptr{Cfloat}, Ptr{Cfloat}, Int64, Cint, Cint, Cint, Cint),
      B, X, R, _cat_codebooks(C), Int64(n), Cint(d), Cint(m), Cint(h), Cint(code_base)))
    return B
  end
  _check(ccall((:rq_encode_opq_i16, librayuela_hip), Cint,
    (Ptr{Int16}, Ptr{Cfloat}, Ptr{Cfloat}, Ptr{Cfloat}, Int64, Cint, Cint, Cint),
    B, X, R, _cat_codebooks(C), Int64(n), Cint(d), Cint(m), Cint(h)))
  return B
end

"""
    groundtruth(Xb::Matrix{Float32}, Xq::Matrix{Float32}, k=1) -> ids, dists
    groundtruth(Xb::Matrix{UInt8}, Xq::Matrix{Float32}, k=1)   -> ids, dists
The exact `k` nearest columns of `Xb` for every column of `Xq`: `ids` is a k x nq `Matrix{Int32}` of one-based ids, nearest first and
ties by id -- what the `*_groundtruth.ivecs` files of src/read_datasets.jl hold and `eval_recall` (src/Linscan.jl:196-234) takes --
and `dists` the squared distances accumulated coordinate by coordinate in Float64.  The reference has no such function.
"""
function groundtruth(Xb::Matrix{Float32}, Xq::Matrix{Float32}, k::Integer=1)
  d, n  = size(Xb)
  nq    = size(Xq, 2)
  @assert size(Xq, 1) == d
  dists = Matrix{Float64}(undef, k, nq)
  ids   = Matrix{UInt32}(undef, k, nq)
  _check(ccall((:rq_knn, librayuela_hip), Cint,
    (Ptr{Cdouble}, Ptr{UInt32}, Ptr{Cfloat}, Ptr{Cfloat}, Int64, Int64, Cint, Cint, Cint),
    dists, ids, Xb, Xq, Int64(n), Int64(nq), Cint(d), Cint(k), Cint(1)))
  return convert(Matrix{Int32}, ids), dists
end

function groundtruth(Xb::Matrix{UInt8}, Xq::Matrix{Float32}, k::Integer=1)
  d, n  = size(Xb)
  nq    = size(Xq, 2)
  @assert size(Xq, 1) == d
  dists = Matrix{Float64}(undef, k, nq)
  ids   = Matrix{UInt32}(undef, k, nq)
  _check(ccall((:rq_knn_bytes, librayuela_hip), Cint,
    (Ptr{Cdouble}, Ptr{UInt32}, Ptr{UInt8}, Ptr{Cfloat}, Int64, Int64, Cint, Cint, Cint),
    dists, ids, Xb, Xq, Int64(n), Int64(nq), Cint(d), Cint(k), Cint(1)))
  return convert(Matrix{Int32}, ids), dists
end

"""
    quantize_pq(X::Matrix{UInt8}, C, V=false) -> B
    quantize_opq(X::Matrix{UInt8}, R, C, V=false) -> B
Byte data as `bvecs_read` returns it (src/xvecs_read.jl:14-52), encoded without the host-side
`convert(Matrix{Float32}, X)` of src/read_datasets.jl:148-167: `B == quantize_pq(convert(Matrix{Float32}, X), C)`,
from a quarter of the bytes over PCIe.
"""
function quantize_pq(X::Matrix{UInt8}, C::Vector{Matrix{Float32}}, V::Bool=false)
  d, n = size(X)
  m    = length(C)
  h    = size(C[1], 2)
  B    = _result(Int16, m, n)
  if V print("Encoding on $m codebooks with librayuela_hip... ") end
  if h > 256      # rq_encode_pq_bytes_wide: the 16-bit codes of the widened rows, from the bytes
    code_base = 1
    _check(ccall((:rq_encode_pq_bytes_wide, librayuela_hip), Cint,
      (Ptr{Int16}, Ptr{UInt8}, Ptr{Cfloat}, Int64, Cint, Cint, Cint, Cint),
      B, X, _cat_codebooks(C), Int64(n), Cint(d), Cint(m), Cint(h), Cint(code_base)))
    if V println("done") end
    return B
  end
  _check(ccall((:rq_encode_pq_bytes_i16, librayuela_hip), Cint,
    (Ptr{Int16}, Ptr{UInt8}, Ptr{Cfloat}, Int64, Cint, Cint, Cint),
    B, X, _cat_codebooks(C), Int64(n), Cint(d), Cint(m), Cint(h)))
  if V println("done") end
  return B
end

function quantize_opq(X::Matrix{UInt8}, R::Matrix{Float32}, C::Vector{Matrix{Float32}}, V::Bool=false)
  d, n = size(X)
  m    = length(C)
  h    = size(C[1], 2)
  B    = _result(Int16, m, n)
  if h > 256      # rq_encode_opq_bytes_wide
    code_base = 1
    _check(ccall((:rq_encode_opq_bytes_wide, librayuela_hip), Cint,
      (Ptr{Int16}, Ptr{UInt8}, Ptr{Cfloat}, Ptr{Cfloat}, Int64, Cint, Cint, Cint, Cint),
      B, X, R, _cat_codebooks(C), Int64(n), Cint(d), Cint(m), Cint(h), Cint(code_base)))
    return B
  end
  _check(ccall((:rq_encode_opq_bytes_i16, librayuela_hip), Cint,
    (Ptr{Int16}, Ptr{UInt8}, Ptr{Cfloat}, Ptr{Cfloat}, Int64, Cint, Cint, Cint),
    B, X, R, _cat_codebooks(C), Int64(n), Cint(d), Cint(m), Cint(h)))
  return B
end

"""
    quantize_rvq(X, C, V=false) -> B, singletons     (src/RVQ.jl:18-66)
`B::Matrix{Int16}` m-by-n one-based; `singletons[i]` holds re-picked entries for the unused centres of
codebook i.  The m encode stages and residual updates run on the device; the library returns the
per-centre counts, and only when some are zero is the reference's own randomised re-pick
(`Clustering.repick_unused_centers`, :50-53; needs `using Clustering, Distances` like src/Rayuela.jl)
replayed here on the residual of that stage.
"""
function quantize_rvq(X::Matrix{Float32}, C::Vector{Matrix{Float32}}, V::Bool=false)
  d, n = size(X)
  m    = length(C)
  h    = size(C[1], 2)
  B      = Matrix{Int16}(undef, m, n)
  counts = Matrix{UInt32}(undef, h, m)          # C view [m][h]
  if h > 256      # rq_encode_rvq_wide: up to 32767 codewords per stage (src/RVQ.jl:60-62)
    code_base = 1
    _check(ccall((:rq_encode_rvq_wide, librayuela_hip), Cint,
      (Ptr{Int16}, Ptr{Cfloat}, Ptr{Cfloat}, Int64, Cint, Cint, Cint, Cint, Ptr{UInt32}, Ptr{Cfloat}),
      B, X, hcat(C...), Int64(n), Cint(d), Cint(m), Cint(h), Cint(code_base), counts, C_NULL))
  else
  _check(ccall((:rq_encode_rvq_i16, librayuela_hip), Cint,
    (Ptr{Int16}, Ptr{Cfloat}, Ptr{Cfloat}, Int64, Cint, Cint, Cint, Ptr{UInt32}, Ptr{Cfloat}),
    B, X, hcat(C...), Int64(n), Cint(d), Cint(m), Cint(h), counts, C_NULL))
  end
  singletons = Vector{Matrix{Float32}}(undef, m)
  if any(counts .== 0)
    Xr = copy(X)
    for i = 1:m
      unused = findall(counts[:, i] .== 0)
      picked = C[i][:, B[i, :]]
      if !isempty(unused)
        costs = vec(sum((Xr .- picked) .^ 2, dims=1))
        temp_codebook = similar(C[i])
        Clustering.repick_unused_centers(Xr, costs, temp_codebook, unused, Distances.SqEuclidean())
        singletons[i] = temp_codebook[:, unused]
      end
      Xr .-= picked
    end
  end
  return B, singletons
end

"""
    quantize_competitiveq(X, C, H; nsplits=1) -> B     (src/CompetitiveQ.jl:75-135 for every column of X)
Beam-search residual encoding: the `H` best partial encodings of each vector survive a stage (1 <= H <= min(32, h)); H = 1 is
`quantize_rvq`.  `B::Matrix{Int16}` m-by-n one-based, in `quantize_rvq`'s layout; h > 256 takes rq_encode_rvq_beam_wide.  `train_competitiveq`
(src/CompetitiveQ.jl:138-221) is a per-sample SGD and is not provided: train with `train_rvq` / `train_ervq`.
"""
function quantize_competitiveq(X::Matrix{Float32}, C::Vector{Matrix{Float32}}, H::Integer; nsplits::Integer=1)
  d, n = size(X)
  m    = length(C)
  h    = size(C[1], 2)
  B    = Matrix{Int16}(undef, m, n)
  if h > 256      # rq_encode_rvq_beam_wide: up to 32767 codewords per stage (src/CompetitiveQ.jl:75-135 on Matrix{Int16})
    code_base = 1
    _check(ccall((:rq_encode_rvq_beam_wide, librayuela_hip), Cint,
      (Ptr{Int16}, Ptr{Cfloat}, Ptr{Cfloat}, Int64, Cint, Cint, Cint, Cint, Cint, Cint, Ptr{Cfloat}, Ptr{Cfloat}),
      B, X, hcat(C...), Int64(n), Cint(d), Cint(m), Cint(h), Cint(H), Cint(nsplits), Cint(code_base), C_NULL, C_NULL))
    return B
  end
  _check(ccall((:rq_encode_rvq_beam_i16, librayuela_hip), Cint,
    (Ptr{Int16}, Ptr{Cfloat}, Ptr{Cfloat}, Int64, Cint, Cint, Cint, Cint, Cint, Ptr{Cfloat}, Ptr{Cfloat}),
    B, X, hcat(C...), Int64(n), Cint(d), Cint(m), Cint(h), Cint(H), Cint(nsplits), C_NULL, C_NULL))
  return B
end

"""
    encode(x, C, new_res, m, h, d, H) -> codes, residual     (src/CompetitiveQ.jl:75-135)
The reference's signature for one vector; `new_res` (its residual buffer) is accepted and ignored.  Not exported: call it
as `RayuelaHIP.encode`.
"""
function encode(x::Vector{Float32}, C::Vector{Matrix{Float32}}, new_res, m::Integer, h::Integer, d::Integer, H::Integer)
  xr    = Vector{Float32}(undef, d)
  if h > 256      # rq_encode_rvq_beam_wide: Int16 codes, one-based as the reference's
    codes1    = Vector{Int16}(undef, m)
    n         = 1
    nsplits   = 1
    code_base = 1
    _check(ccall((:rq_encode_rvq_beam_wide, librayuela_hip), Cint,
      (Ptr{Int16}, Ptr{Cfloat}, Ptr{Cfloat}, Int64, Cint, Cint, Cint, Cint, Cint, Cint, Ptr{Cfloat}, Ptr{Cfloat}),
      codes1, x, hcat(C...), Int64(n), Cint(d), Cint(m), Cint(h), Cint(H), Cint(nsplits), Cint(code_base), C_NULL, xr))
    return codes1, xr
  end
  codes = Vector{UInt8}(undef, m)
  _check(ccall((:rq_encode_rvq_beam, librayuela_hip), Cint,
    (Ptr{UInt8}, Ptr{Cfloat}, Ptr{Cfloat}, Int64, Cint, Cint, Cint, Cint, Cint, Ptr{Cfloat}, Ptr{Cfloat}),
    codes, x, hcat(C...), Int64(1), Cint(d), Cint(m), Cint(h), Cint(H), Cint(1), C_NULL, xr))
  return Int16.(codes) .+ Int16(1), xr
end

"""milliseconds of this thread's last beam call: (stage kernels, expand kernels, other)"""
function last_beam_timing()
  ms  = zeros(Cdouble, 3)
  cap = 3
  _check(ccall((:rq_last_beam_timing, librayuela_hip), Cint, (Ptr{Cdouble}, Cint), ms, Cint(cap)))
  return (stage=ms[1], expand=ms[2], other=ms[3])
end

"""
    train_rvq(X, m, h, niter=25, V=false; seed=0) -> C, B, error     (src/RVQ.jl:86-127)
One k-means per stage on the running residual, on the device, seeded by kmeans++ like the reference's
`kmeans(Xr, h, init=:kmpp, maxiter=niter)` -- with the library's seeded stream instead of Julia's RNG, so runs
agree in objective, not bit for bit (and are bit-reproducible for a given `seed`).
"""
function train_rvq(X::Matrix{Float32}, m::Integer, h::Integer, niter::Integer=25, V::Bool=false; seed::Integer=0)
  d, n = size(X)
  Ccat = Array{Float32}(undef, d, h, m)            # C view [m][h][d]
  B    = _result(Int16, m, n)
  err  = Ref{Cdouble}(0.0)
  if h > 256      # more than 256 codewords per stage: the same loop on 16-bit codes, rq_train_rvq_wide
    code_base = 1
    _check(ccall((:rq_train_rvq_wide, librayuela_hip), Cint,
      (Ptr{Cfloat}, Ptr{Int16}, Ref{Cdouble}, Ptr{Cfloat}, Int64, Cint, Cint, Cint, Cint, UInt64, Cint),
      Ccat, B, err, X, Int64(n), Cint(d), Cint(m), Cint(h), Cint(niter), UInt64(seed), Cint(code_base)))
    return [Ccat[:, :, i] for i = 1:m], B, Float32(err[])
  end
  _check(ccall((:rq_train_rvq, librayuela_hip), Cint,
    (Ptr{Cfloat}, Ptr{Int16}, Ref{Cdouble}, Ptr{Cfloat}, Int64, Cint, Cint, Cint, Cint, UInt64),
    Ccat, B, err, X, Int64(n), Cint(d), Cint(m), Cint(h), Cint(niter), UInt64(seed)))
  C = [Ccat[:, :, i] for i = 1:m]
  return C, B, Float32(err[])
end

"""
    quantize_ervq(X, C, V=false) -> B, singletons     (src/ERVQ.jl:19-26): identical to quantize_rvq
"""
quantize_ervq(X::Matrix{Float32}, C::Vector{Matrix{Float32}}, V::Bool=false) = quantize_rvq(X, C, V)

"""
    train_ervq(X, B, C, m, h, niter=25, V=false; seed=0) -> C, B, error     (src/ERVQ.jl:51-135)
Enhanced RVQ / Stacked Quantizers, device-resident (rq_train_ervq; rq_train_ervq_wide when h > 256): per iteration and codebook j, the codebook update,
the refill of entries without rows, the re-encode of stages j..m and the error.  `B` is any integer m-by-n matrix of
one-based codes; the result is `Matrix{Int16}` and equals `quantize_ervq(X, C)[1]`.  The reference prints `Qerror is ...`
after every step; here `V=true` prints those lines from the recorded trace.  Entries without rows are re-drawn by
Clustering's rule from the library's stream seeded by `seed` (the reference: Julia's RNG), for the first codebook too.
"""
function train_ervq(X::Matrix{Float32}, B::Matrix{T2}, C::Vector{Matrix{Float32}}, m::Integer, h::Integer,
                    niter::Integer=25, V::Bool=false; seed::Integer=0) where T2 <: Integer
  d, n = size(X)
  @assert size(B) == (m, n) && length(C) == m && all(size(Ci) == (d, h) for Ci in C)
  Ccat = Array{Float32}(undef, d, h, m)            # C view [m][h][d]
  for i = 1:m
    Ccat[:, :, i] = C[i]
  end
  B1  = convert(Matrix{Int16}, B)
  B1 === B && (B1 = copy(B))
  err = Ref{Cdouble}(0.0)
  obj = Vector{Cdouble}(undef, niter * m + 1)
  if h > 256      # more than 256 entries per codebook: the same loop on 16-bit codes, rq_train_ervq_wide (src/ERVQ.jl:51-135)
    code_base = 1
    _check(ccall((:rq_train_ervq_wide, librayuela_hip), Cint,
      (Ptr{Cfloat}, Ptr{Int16}, Ref{Cdouble}, Ptr{Cdouble}, Ptr{Cfloat}, Int64, Cint, Cint, Cint, Cint, UInt64, Cint),
      Ccat, B1, err, obj, X, Int64(n), Cint(d), Cint(m), Cint(h), Cint(niter), UInt64(seed), Cint(code_base)))
  else
  _check(ccall((:rq_train_ervq, librayuela_hip), Cint,
    (Ptr{Cfloat}, Ptr{Int16}, Ref{Cdouble}, Ptr{Cdouble}, Ptr{Cfloat}, Int64, Cint, Cint, Cint, Cint, UInt64),
    Ccat, B1, err, obj, X, Int64(n), Cint(d), Cint(m), Cint(h), Cint(niter), UInt64(seed)))
  end
  if V
    print("Error after init is $(obj[1]) \n")
    for i = 1:niter
      print("=== Iteration $i / $niter ===\n")
      for j = 1:m
        print("Updating codebook $j... done.\nUpdating codes... done. Qerror is $(obj[1 + (i - 1) * m + j]).\n")
      end
    end
  end
  return [Ccat[:, :, i] for i = 1:m], B1, Float32(err[])
end

"""
    train_ervq(X, m, h, niter=25, V=false; seed=0) -> C, B, error     (src/ERVQ.jl:138-148): initialised by train_rvq
"""
function train_ervq(X::Matrix{Float32}, m::Integer, h::Integer, niter::Integer=25, V::Bool=false; seed::Integer=0)
  C, B, _ = train_rvq(X, m, h, niter, V; seed=seed)
  train_ervq(X, B, C, m, h, niter, V; seed=seed)
end

"""
    linscan_pq(B, X, C, b, k=10000) -> dists, idx     (src/Linscan.jl:5-26)
`B::Matrix{UInt8}` zero-based m-by-n; returns k-by-nq `dists::Matrix{Cfloat}` (ascending) and
`idx::Matrix{Cuint}` ONE-based (the reference's `res .+= 1` is folded into the kernel: id_base = 1).
"""
function linscan_pq(B::Matrix{UInt8}, X::Matrix{Cfloat}, C::Vector{Matrix{Cfloat}}, b::Int, k::Int=10000)
  m, n  = size(B)
  d, nq = size(X)
  @show k, nq
  dists = _result(Cfloat, k, nq)
  res   = _result(Cuint,  k, nq)
  _check(ccall((:rq_linscan_pq, librayuela_hip), Cint,
    (Ptr{Cfloat}, Ptr{Cuint}, Ptr{Cuchar}, Ptr{Cfloat}, Ptr{Cfloat}, Int64, Int64, Cint, Cint, Cint, Cint),
    dists, res, B, cat(C..., dims=3), X, Int64(n), Int64(nq), Cint(m), Cint(d), Cint(k), Cint(1)))
  return dists, res
end

function linscan_pq(B::Matrix{T}, X::Matrix{Cfloat}, C::Vector{Matrix{Cfloat}}, b::Int, k::Int=10000) where T <: Integer
  h = size(C[1], 2)
  if h > 256      # 16-bit codes (quantize_pq at h > 256): rq_linscan_pq_wide; `b` is accepted and not interpreted
    m, n  = size(B)
    d, nq = size(X)
    B16   = convert(Matrix{Int16}, B)            # one-based, as quantize_pq returns them: code_base = 1
    dists = _result(Cfloat, k, nq)
    res   = _result(Cuint,  k, nq)
    code_base = 1
    id_base   = 1
    _check(ccall((:rq_linscan_pq_wide, librayuela_hip), Cint,
      (Ptr{Cfloat}, Ptr{Cuint}, Ptr{Int16}, Ptr{Cfloat}, Ptr{Cfloat}, Int64, Int64, Cint, Cint, Cint, Cint, Cint, Cint),
      dists, res, B16, cat(C..., dims=3), X, Int64(n), Int64(nq), Cint(m), Cint(h), Cint(d), Cint(k), Cint(code_base),
      Cint(id_base)))
    return dists, res
  end
  B_uint8 = convert(Matrix{UInt8}, B .- 1)      # src/Linscan.jl:35
  return linscan_pq(B_uint8, X, C, b, k)
end

"""
    linscan_opq(B, X, C, b, R, k=10000)     (src/Linscan.jl:93-115) == linscan_pq(B, R' * X, C, b, k)
"""
function linscan_opq(B::Matrix{UInt8}, X::Matrix{Cfloat}, C::Vector{Matrix{Cfloat}}, b::Int,
                     R::Matrix{Cfloat}, k::Int=10000)
  m, n  = size(B)
  d, nq = size(X)
  dists = _result(Cfloat, k, nq)
  res   = _result(Cuint,  k, nq)
  _check(ccall((:rq_linscan_opq, librayuela_hip), Cint,
    (Ptr{Cfloat}, Ptr{Cuint}, Ptr{Cuchar}, Ptr{Cfloat}, Ptr{Cfloat}, Ptr{Cfloat}, Int64, Int64, Cint, Cint, Cint, Cint),
    dists, res, B, cat(C..., dims=3), X, R, Int64(n), Int64(nq), Cint(m), Cint(d), Cint(k), Cint(1)))
  return dists, res
end

function linscan_opq(B::Matrix{T}, X::Matrix{Cfloat}, C::Vector{Matrix{Cfloat}}, b::Int,
                     R::Matrix{Cfloat}, k::Int=10000) where T <: Integer
  h = size(C[1], 2)
  if h > 256      # 16-bit codes (quantize_opq at h > 256): rq_linscan_opq_wide; `b` is accepted and not interpreted
    m, n  = size(B)
    d, nq = size(X)
    B16   = convert(Matrix{Int16}, B)
    dists = _result(Cfloat, k, nq)
    res   = _result(Cuint,  k, nq)
    code_base = 1
    id_base   = 1
    _check(ccall((:rq_linscan_opq_wide, librayuela_hip), Cint,
      (Ptr{Cfloat}, Ptr{Cuint}, Ptr{Int16}, Ptr{Cfloat}, Ptr{Cfloat}, Ptr{Cfloat}, Int64, Int64, Cint, Cint, Cint, Cint, Cint,
       Cint),
      dists, res, B16, cat(C..., dims=3), X, R, Int64(n), Int64(nq), Cint(m), Cint(h), Cint(d), Cint(k), Cint(code_base),
      Cint(id_base)))
    return dists, res
  end
  B_uint8 = convert(Matrix{UInt8}, B .- 1)
  return linscan_opq(B_uint8, X, C, b, R, k)
end

"""
    linscan_lsq(B, X, C, dbnorms, R, k=10000) -> dists, idx     (src/Linscan.jl:118-157)
ADC search for additive quantizers, database norms passed apart; `idx` is ONE-based as in the reference.
"""
function linscan_lsq(B::Matrix{UInt8}, X::Matrix{Cfloat}, C::Vector{Matrix{Cfloat}},
                     dbnorms::Vector{Cfloat}, R::Matrix{Cfloat}, k::Int=10000)
  m, n  = size(B)
  d, nq = size(X)
  _, h  = size(C[1])
  dists = _result(Cfloat, k, nq)
  res   = _result(Cuint,  k, nq)
  _check(ccall((:rq_linscan_lsq, librayuela_hip), Cint,
    (Ptr{Cfloat}, Ptr{Cuint}, Ptr{Cuchar}, Ptr{Cfloat}, Ptr{Cfloat}, Ptr{Cfloat}, Ptr{Cfloat},
     Int64, Int64, Cint, Cint, Cint, Cint, Cint),
    dists, res, B, X, hcat(C...), dbnorms, R, Int64(n), Int64(nq), Cint(m), Cint(h), Cint(d), Cint(k), Cint(1)))
  return dists, res
end

function linscan_lsq(B::Matrix{T}, X::Matrix{Cfloat}, C::Vector{Matrix{Cfloat}},
                     dbnorms::Vector{Cfloat}, R::Matrix{Cfloat}, k::Int=10000) where T <: Integer
  d, h = size(C[1])
  if h > 256      # 16-bit codes (train_rvq / quantize_rvq at h > 256): rq_linscan_lsq_wide
    m, n  = size(B)
    _, nq = size(X)
    B16   = convert(Matrix{Int16}, B)            # one-based, as quantize_rvq returns them: code_base = 1
    dists = _result(Cfloat, k, nq)
    res   = _result(Cuint,  k, nq)
    code_base = 1
    id_base   = 1
    _check(ccall((:rq_linscan_lsq_wide, librayuela_hip), Cint,
      (Ptr{Cfloat}, Ptr{Cuint}, Ptr{Int16}, Ptr{Cfloat}, Ptr{Cfloat}, Ptr{Cfloat}, Ptr{Cfloat},
       Int64, Int64, Cint, Cint, Cint, Cint, Cint, Cint),
      dists, res, B16, X, hcat(C...), dbnorms, R, Int64(n), Int64(nq), Cint(m), Cint(h), Cint(d), Cint(k), Cint(code_base),
      Cint(id_base)))
    return dists, res
  end
  return linscan_lsq(convert(Matrix{UInt8}, B .- 1), X, C, dbnorms, R, k)
end

"""
    HipLsqIndex(B, C, dbnorms)  /  search(ix, X, R, k=10000) -> dists, idx
linscan_lsq over a PREPARED base (rq_lsq_prepare / rq_lsq_search / rq_lsq_release): codes, dbnorms and codebooks stay on the
device together with the pre-filter's O(n) pass over the base, which `linscan_lsq` repeats on every call.  `search` returns
exactly what `linscan_lsq(B, X, C, dbnorms, R, k)` returns (one-based `idx`).
"""
mutable struct HipLsqIndex
  handle::Ptr{Cvoid}
  n::Int
  m::Int
  d::Int
  function HipLsqIndex(B::Matrix{UInt8}, C::Vector{Matrix{Cfloat}}, dbnorms::Vector{Cfloat})
    m, n = size(B)
    d, h = size(C[1])
    hd = ccall((:rq_lsq_prepare, librayuela_hip), Ptr{Cvoid},
               (Ptr{Cuchar}, Ptr{Cfloat}, Ptr{Cfloat}, Int64, Cint, Cint, Cint),
               B, hcat(C...), dbnorms, Int64(n), Cint(m), Cint(h), Cint(d))
    hd == C_NULL && error("rq_lsq_prepare: " * unsafe_string(ccall((:rq_last_error, librayuela_hip), Cstring, ())))
    ix = new(hd, n, m, d)
    finalizer(x -> (x.handle != C_NULL && ccall((:rq_lsq_release, librayuela_hip), Cvoid, (Ptr{Cvoid},), x.handle); x.handle = C_NULL), ix)
    return ix
  end
end
HipLsqIndex(B::Matrix{T}, C::Vector{Matrix{Cfloat}}, dbnorms::Vector{Cfloat}) where T <: Integer =
  HipLsqIndex(convert(Matrix{UInt8}, B .- 1), C, dbnorms)

function search(ix::HipLsqIndex, X::Matrix{Cfloat}, R::Matrix{Cfloat}, k::Int=10000)
  d, nq = size(X)
  dists = _result(Cfloat, k, nq)
  res   = _result(Cuint,  k, nq)
  _check(ccall((:rq_lsq_search, librayuela_hip), Cint,
    (Ptr{Cvoid}, Ptr{Cfloat}, Ptr{Cuint}, Ptr{Cfloat}, Ptr{Cfloat}, Int64, Cint, Cint),
    ix.handle, dists, res, X, R, Int64(nq), Cint(k), Cint(1)))
  return dists, res
end

"""
    get_norms_codebook(B, C; niter=100, seed=0) -> norms_codes, norms_codebook     (src/utils.jl:4-26)
The norms of the reconstructions, computed on the device and clustered there by a 1-D k-means with h centres
(rq_get_norms_codebook); `norms_codes` are the k-means' final assignments, one-based.  `niter` = 100 is Clustering's default
`maxiter` as recalled; `seed` feeds the library's stream where the reference draws from Julia's global RNG.
"""
function get_norms_codebook(B::Matrix{UInt8}, C::Vector{Matrix{Cfloat}}; niter::Integer=100, seed::Integer=0)
  m, n = size(B)
  d, h = size(C[1])
  hn = h
  norm_codes = Vector{UInt8}(undef, n)
  cbnorms    = Vector{Cfloat}(undef, hn)
  _check(ccall((:rq_get_norms_codebook, librayuela_hip), Cint,
    (Ptr{Cuchar}, Ptr{Cfloat}, Ptr{Cfloat}, Ptr{Cuchar}, Ptr{Cfloat}, Int64, Cint, Cint, Cint, Cint, Cint, UInt64),
    norm_codes, cbnorms, C_NULL, B, hcat(C...), Int64(n), Cint(d), Cint(m), Cint(h), Cint(hn), Cint(niter), UInt64(seed)))
  return convert(Vector{Int}, norm_codes) .+ 1, cbnorms
end
function get_norms_codebook(B::Matrix{T}, C::Vector{Matrix{Cfloat}}; niter::Integer=100, seed::Integer=0) where T <: Integer
  d, h = size(C[1])
  if h > 256      # 16-bit codes and a norms codebook of h entries: rq_get_norms_codebook_wide
    m, n = size(B)
    hn = h
    B16 = convert(Matrix{Int16}, B)
    norm_codes = Vector{Int16}(undef, n)
    cbnorms    = Vector{Cfloat}(undef, hn)
    code_base = 1
    _check(ccall((:rq_get_norms_codebook_wide, librayuela_hip), Cint,
      (Ptr{Int16}, Ptr{Cfloat}, Ptr{Cfloat}, Ptr{Int16}, Ptr{Cfloat}, Int64, Cint, Cint, Cint, Cint, Cint, UInt64, Cint),
      norm_codes, cbnorms, C_NULL, B16, hcat(C...), Int64(n), Cint(d), Cint(m), Cint(h), Cint(hn), Cint(niter), UInt64(seed),
      Cint(code_base)))
    return convert(Vector{Int}, norm_codes) .+ 1, cbnorms
  end
  return get_norms_codebook(convert(Matrix{UInt8}, B .- 1), C; niter=niter, seed=seed)
end

"""
    quantize_norms(B, C, cbnorms) -> dbnormsB, dbnormsX     (src/utils.jl:29-59)
For every column of B the first entry of `cbnorms` nearest to the norm of its reconstruction ((norm - c)^2 in Float32,
findmin's tie rule), one-based, and the norms themselves (rq_quantize_norms).
"""
function quantize_norms(B::Matrix{UInt8}, C::Vector{Matrix{Cfloat}}, cbnorms::Vector{Cfloat})
  m, n = size(B)
  d, h = size(C[1])
  hn = length(cbnorms)
  norm_codes = Vector{UInt8}(undef, n)
  dbnormsX   = Vector{Cfloat}(undef, n)
  _check(ccall((:rq_quantize_norms, librayuela_hip), Cint,
    (Ptr{Cuchar}, Ptr{Cfloat}, Ptr{Cuchar}, Ptr{Cfloat}, Ptr{Cfloat}, Int64, Cint, Cint, Cint, Cint),
    norm_codes, dbnormsX, B, hcat(C...), cbnorms, Int64(n), Cint(d), Cint(m), Cint(h), Cint(hn)))
  return convert(Vector{Int16}, norm_codes) .+ Int16(1), dbnormsX
end
function quantize_norms(B::Matrix{T}, C::Vector{Matrix{Cfloat}}, cbnorms::Vector{Cfloat}) where T <: Integer
  d, h = size(C[1])
  if h > 256      # 16-bit codes, cbnorms of up to 32767 entries: rq_quantize_norms_wide
    m, n = size(B)
    hn = length(cbnorms)
    B16 = convert(Matrix{Int16}, B)
    norm_codes = Vector{Int16}(undef, n)
    dbnormsX   = Vector{Cfloat}(undef, n)
    code_base = 1
    _check(ccall((:rq_quantize_norms_wide, librayuela_hip), Cint,
      (Ptr{Int16}, Ptr{Cfloat}, Ptr{Int16}, Ptr{Cfloat}, Ptr{Cfloat}, Int64, Cint, Cint, Cint, Cint, Cint),
      norm_codes, dbnormsX, B16, hcat(C...), cbnorms, Int64(n), Cint(d), Cint(m), Cint(h), Cint(hn), Cint(code_base)))
    return norm_codes .+ Int16(1), dbnormsX
  end
  return quantize_norms(convert(Matrix{UInt8}, B .- 1), C, cbnorms)
end

"""
    linscan_cq(B, X, C, k=10000) -> dists, idx     (src/Linscan.jl:160-193)
"""
function linscan_cq(B::Matrix{UInt8}, X::Matrix{Cfloat}, C::Vector{Matrix{Cfloat}}, k::Int=10000)
  m, n  = size(B)
  d, nq = size(X)
  _, h  = size(C[1])
  dists = _result(Cfloat, k, nq)
  res   = _result(Cuint,  k, nq)
  _check(ccall((:rq_linscan_cq, librayuela_hip), Cint,
    (Ptr{Cfloat}, Ptr{Cuint}, Ptr{Cuchar}, Ptr{Cfloat}, Ptr{Cfloat}, Int64, Int64, Cint, Cint, Cint, Cint, Cint),
    dists, res, B, X, hcat(C...), Int64(n), Int64(nq), Cint(m), Cint(h), Cint(d), Cint(k), Cint(1)))
  return dists, res
end

function linscan_cq(B::Matrix{T}, X::Matrix{Cfloat}, C::Vector{Matrix{Cfloat}}, k::Int=10000) where T <: Integer
  d, h = size(C[1])
  if h > 256      # 16-bit codes: rq_linscan_cq_wide
    m, n  = size(B)
    _, nq = size(X)
    B16   = convert(Matrix{Int16}, B)
    dists = _result(Cfloat, k, nq)
    res   = _result(Cuint,  k, nq)
    code_base = 1
    id_base   = 1
    _check(ccall((:rq_linscan_cq_wide, librayuela_hip), Cint,
      (Ptr{Cfloat}, Ptr{Cuint}, Ptr{Int16}, Ptr{Cfloat}, Ptr{Cfloat}, Int64, Int64, Cint, Cint, Cint, Cint, Cint, Cint),
      dists, res, B16, X, hcat(C...), Int64(n), Int64(nq), Cint(m), Cint(h), Cint(d), Cint(k), Cint(code_base), Cint(id_base)))
    return dists, res
  end
  return linscan_cq(convert(Matrix{UInt8}, B .- 1), X, C, k)
end

# splitarray(1:d, m) sizes (src/utils.jl:179-203), to cut the flat codebook buffer back into matrices
function _split_codebooks(Ccat::Vector{Float32}, d::Int, m::Int, h::Int)
  per, extra = divrem(d, m)
  C = Vector{Matrix{Float32}}(undef, m)
  pos = 0
  for i = 1:m
    sub  = per + (i <= extra ? 1 : 0)
    C[i] = reshape(Ccat[pos+1 : pos+sub*h], sub, h)
    pos += sub * h
  end
  return C
end

"""
    train_pq(X, m, h, niter=25, V=false) -> C, B, error     (src/PQ.jl:68-99)
k-means per subspace on the device, kmeans++ seeding (`init=:kmpp`, src/PQ.jl:86) from the library's seeded stream.
"""
function train_pq(X::Matrix{Float32}, m::Integer, h::Integer, niter::Integer=25, V::Bool=false; seed::Integer=0)
  d, n = size(X)
  Ccat = Vector{Float32}(undef, h * d)
  B    = _result(Int16, m, n)
  err  = Ref{Cdouble}(0.0)
  if h > 256      # more than 256 codewords per codebook: the same loop on 16-bit codes, rq_train_pq_wide
    code_base = 1
    _check(ccall((:rq_train_pq_wide, librayuela_hip), Cint,
      (Ptr{Cfloat}, Ptr{Int16}, Ref{Cdouble}, Ptr{Cfloat}, Int64, Cint, Cint, Cint, Cint, UInt64, Cint),
      Ccat, B, err, X, Int64(n), Cint(d), Cint(m), Cint(h), Cint(niter), UInt64(seed), Cint(code_base)))
    return _split_codebooks(Ccat, d, Int(m), Int(h)), B, Float32(err[])
  end
  _check(ccall((:rq_train_pq, librayuela_hip), Cint,
    (Ptr{Cfloat}, Ptr{Int16}, Ref{Cdouble}, Ptr{Cfloat}, Int64, Cint, Cint, Cint, Cint, UInt64),
    Ccat, B, err, X, Int64(n), Cint(d), Cint(m), Cint(h), Cint(niter), UInt64(seed)))
  return _split_codebooks(Ccat, d, Int(m), Int(h)), B, Float32(err[])
end

"""
    train_opq(X, m, h, niter, init, V=false) -> C, B, R, obj     (src/OPQ.jl:49-139)
"""
function train_opq(X::Matrix{Float32}, m::Integer, h::Integer, niter::Integer, init::String, V::Bool=false; seed::Integer=0)
  d, n = size(X)
  init in ("natural", "random") || error("Intialization $init unknown")   # src/OPQ.jl:74
  Ccat = Vector{Float32}(undef, h * d)
  B    = _result(Int16, m, n)
  R    = Matrix{Float32}(undef, d, d)
  obj  = zeros(Float32, niter + 1)
  if h > 256      # more than 256 codewords per codebook: the same loop on 16-bit codes, rq_train_opq_wide
    code_base = 1
    _check(ccall((:rq_train_opq_wide, librayuela_hip), Cint,
      (Ptr{Cfloat}, Ptr{Int16}, Ptr{Cfloat}, Ptr{Cfloat}, Ptr{Cfloat}, Int64, Cint, Cint, Cint, Cint, Cint, UInt64,
       Ptr{Cfloat}, Ptr{Cfloat}, Cint),
      Ccat, B, R, obj, X, Int64(n), Cint(d), Cint(m), Cint(h), Cint(niter), Cint(init == "natural" ? 0 : 1),
      UInt64(seed), C_NULL, C_NULL, Cint(code_base)))
    return _split_codebooks(Ccat, d, Int(m), Int(h)), B, R, obj
  end
  _check(ccall((:rq_train_opq, librayuela_hip), Cint,
    (Ptr{Cfloat}, Ptr{Int16}, Ptr{Cfloat}, Ptr{Cfloat}, Ptr{Cfloat}, Int64, Cint, Cint, Cint, Cint, Cint, UInt64,
     Ptr{Cfloat}, Ptr{Cfloat}),
    Ccat, B, R, obj, X, Int64(n), Cint(d), Cint(m), Cint(h), Cint(niter), Cint(init == "natural" ? 0 : 1),
    UInt64(seed), C_NULL, C_NULL))
  return _split_codebooks(Ccat, d, Int(m), Int(h)), B, R, obj
end

# ---- resident handles (no counterpart in the reference: they remove its per-call marshalling) ----------------

"""
    HipIndex(C, d; devices=nothing)
Codes uploaded once, searched many times.  `devices = [0, 1, ...]`: one row shard per entry (RCCL gather of the
per-shard top-k + merge inside the library); `nothing`: the current device.  `search` returns what `linscan_pq`
returns (k-by-nq `dists`, ONE-based `idx`).
"""
mutable struct HipIndex
  h::Ptr{Cvoid}
  m::Int
  d::Int
  function HipIndex(C::Vector{Matrix{Cfloat}}, d::Int; devices::Union{Nothing,Vector{<:Integer}}=nothing)
    m = length(C)
    cen = cat(C..., dims=3)
    h = devices === nothing ?
      ccall((:rq_index_create, librayuela_hip), Ptr{Cvoid}, (Cint, Cint, Ptr{Cfloat}), Cint(m), Cint(d), cen) :
      ccall((:rq_index_create_sharded, librayuela_hip), Ptr{Cvoid}, (Cint, Cint, Ptr{Cfloat}, Ptr{Cint}, Cint),
            Cint(m), Cint(d), cen, convert(Vector{Cint}, devices), Cint(length(devices)))
    h == C_NULL && error("rq_index_create: " * unsafe_string(ccall((:rq_last_error, librayuela_hip), Cstring, ())))
    ix = new(h, m, d)
    finalizer(x -> (x.h != C_NULL && ccall((:rq_index_destroy, librayuela_hip), Cvoid, (Ptr{Cvoid},), x.h); x.h = C_NULL), ix)
    return ix
  end
end

function set_codes!(ix::HipIndex, B::Matrix{UInt8}; id_offset::Integer=0)      # B zero-based m-by-n
  _check(ccall((:rq_index_set_codes, librayuela_hip), Cint, (Ptr{Cvoid}, Ptr{Cuchar}, Int64, UInt32),
               ix.h, B, Int64(size(B, 2)), UInt32(id_offset)))
  return ix
end
set_codes!(ix::HipIndex, B::Matrix{T}; id_offset::Integer=0) where T <: Integer =
  set_codes!(ix, convert(Matrix{UInt8}, B .- 1); id_offset=id_offset)

function set_codes_synth!(ix::HipIndex, n::Integer, seed::Integer; id_offset::Integer=0)
  _check(ccall((:rq_index_set_codes_synth, librayuela_hip), Cint, (Ptr{Cvoid}, Int64, UInt64, UInt32),
               ix.h, Int64(n), UInt64(seed), UInt32(id_offset)))
  return ix
end

search(ix::HipIndex, X::Matrix{Cfloat}, k::Int=10000; R::Union{Nothing,Matrix{Cfloat}}=nothing) = _index_search(ix, X, k, R)

function _index_search(ix, X::Matrix{Cfloat}, k::Int, R::Union{Nothing,Matrix{Cfloat}})    # ix: HipIndex or HipIndexU16
  d, nq = size(X)
  dists = Matrix{Cfloat}(undef, k, nq)
  res   = Matrix{Cuint}(undef, k, nq)
  if R === nothing
    _check(ccall((:rq_index_search, librayuela_hip), Cint,
      (Ptr{Cvoid}, Ptr{Cfloat}, Ptr{Cuint}, Ptr{Cfloat}, Int64, Cint, Cint), ix.h, dists, res, X, Int64(nq), Cint(k), Cint(1)))
  else
    _check(ccall((:rq_index_search_opq, librayuela_hip), Cint,
      (Ptr{Cvoid}, Ptr{Cfloat}, Ptr{Cuint}, Ptr{Cfloat}, Ptr{Cfloat}, Int64, Cint, Cint),
      ix.h, dists, res, X, R, Int64(nq), Cint(k), Cint(1)))
  end
  return dists, res
end

"""
    HipIndexU16(C, d; devices=nothing)
`HipIndex` over 16-bit codes: `C` holds m codebooks of `d/m`-by-h centers with any 1 <= h <= 32767 (1 <= m <= 32).
`set_codes!` takes `Matrix{Int16}` (m-by-n) ZERO-based, or any other integer matrix ONE-based; `search` returns what
`linscan_pq` / `linscan_opq` over such codes return (k-by-nq `dists`, ONE-based `idx`).
"""
mutable struct HipIndexU16
  h::Ptr{Cvoid}
  m::Int
  d::Int
  function HipIndexU16(C::Vector{Matrix{Cfloat}}, d::Int; devices::Union{Nothing,Vector{<:Integer}}=nothing)
    m = length(C)
    h = size(C[1], 2)
    cen = cat(C..., dims=3)
    ptr = devices === nothing ?
      ccall((:rq_index_create_wide, librayuela_hip), Ptr{Cvoid}, (Cint, Cint, Cint, Ptr{Cfloat}), Cint(m), Cint(h), Cint(d), cen) :
      ccall((:rq_index_create_sharded_wide, librayuela_hip), Ptr{Cvoid}, (Cint, Cint, Cint, Ptr{Cfloat}, Ptr{Cint}, Cint),
            Cint(m), Cint(h), Cint(d), cen, convert(Vector{Cint}, devices), Cint(length(devices)))
    ptr == C_NULL && error("rq_index_create_wide: " * unsafe_string(ccall((:rq_last_error, librayuela_hip), Cstring, ())))
    ix = new(ptr, m, d)
    finalizer(x -> (x.h != C_NULL && ccall((:rq_index_destroy, librayuela_hip), Cvoid, (Ptr{Cvoid},), x.h); x.h = C_NULL), ix)
    return ix
  end
end

function set_codes!(ix::HipIndexU16, B::Matrix{Int16}; code_base::Integer=0, id_offset::Integer=0)
  _check(ccall((:rq_index_set_codes_wide, librayuela_hip), Cint, (Ptr{Cvoid}, Ptr{Int16}, Int64, Cint, UInt32),
               ix.h, B, Int64(size(B, 2)), Cint(code_base), UInt32(id_offset)))
  return ix
end
set_codes!(ix::HipIndexU16, B::Matrix{T}; id_offset::Integer=0) where T <: Integer =
  set_codes!(ix, convert(Matrix{Int16}, B); code_base=1, id_offset=id_offset)

search(ix::HipIndexU16, X::Matrix{Cfloat}, k::Int=10000; R::Union{Nothing,Matrix{Cfloat}}=nothing) = _index_search(ix, X, k, R)

"""
    HipIvfIndex(Q, C; by_residual=true)
IVFADC (Jegou et al., PAMI 2011; no counterpart in the reference): `Q` holds the `d`-by-nlist coarse centroids (1 <= nlist <= 32767),
`C` the m `d/m`-by-256 codebooks of the encoded vector -- the residual `x - Q[:, list(x)]` with `by_residual`, else `x`.
`build!(ix, X; id_offset=0)` assigns, encodes and groups the columns of `X` on the device; `search(ix, X, nprobe, k)` scans the
`nprobe` nearest lists of every query and returns k-by-nq `dists` and ONE-based `idx`, a union of fewer than k rows ending in
`(NaN, 0)`.  `train_ivfpq(X, nlist, m)` gives `Q` and `C`.  include/rayuela_hip.h states the arithmetic.
"""
mutable struct HipIvfIndex
  h::Ptr{Cvoid}
  m::Int
  d::Int
  nlist::Int
  function HipIvfIndex(Q::Matrix{Cfloat}, C::Vector{Matrix{Cfloat}}; by_residual::Bool=true)
    d, nlist = size(Q)
    m = length(C)
    d % m == 0 || error("d=$d is not a multiple of m=$m")
    cen = cat(C..., dims=3)
    h = ccall((:rq_ivf_create, librayuela_hip), Ptr{Cvoid}, (Cint, Cint, Ptr{Cfloat}, Cint, Ptr{Cfloat}, Cint),
              Cint(d), Cint(nlist), Q, Cint(m), cen, Cint(by_residual))
    h == C_NULL && error("rq_ivf_create: " * unsafe_string(ccall((:rq_last_error, librayuela_hip), Cstring, ())))
    ix = new(h, m, d, nlist)
    finalizer(x -> (x.h != C_NULL && ccall((:rq_ivf_destroy, librayuela_hip), Cvoid, (Ptr{Cvoid},), x.h); x.h = C_NULL), ix)
    return ix
  end
end

function build!(ix::HipIvfIndex, X::Matrix{Cfloat}; id_offset::Integer=0)
  d, n = size(X)
  d == ix.d || error("X must have d=$(ix.d) rows")
  _check(ccall((:rq_ivf_build, librayuela_hip), Cint, (Ptr{Cvoid}, Ptr{Cfloat}, Int64, UInt32),
               ix.h, X, Int64(n), UInt32(id_offset)))
  return ix
end

function build!(ix::HipIvfIndex, X::Matrix{UInt8}; id_offset::Integer=0)
  d, n = size(X)
  d == ix.d || error("X must have d=$(ix.d) rows")
  _check(ccall((:rq_ivf_build_bytes, librayuela_hip), Cint, (Ptr{Cvoid}, Ptr{UInt8}, Int64, UInt32),
               ix.h, X, Int64(n), UInt32(id_offset)))
  return ix
end

# the least id_offset an add may take: the largest id loaded plus one, 0 for an index with no base
function _ivf_next_id(ix::HipIvfIndex)
  out = zeros(Int64, 12)
  cap = length(out)
  _check(ccall((:rq_ivf_info, librayuela_hip), Cint, (Ptr{Cvoid}, Ptr{Int64}, Cint), ix.h, out, Cint(cap)))
  return out[12]
end

"""
    add!(ix, X; id_offset=nothing)
    add_codes!(ix, lists, B; id_offset=nothing)
Put the columns of `X` (`Matrix{Cfloat}` or `Matrix{UInt8}`), or rows given as zero-based `lists` and m-by-n zero-based codes `B`,
BEHIND the loaded base of a `HipIvfIndex`: afterwards the index holds what one `build!` of all columns would have loaded.
`id_offset` (`nothing`: the next id) must not lie below the largest id loaded plus one; gaps are allowed.
"""
function add!(ix::HipIvfIndex, X::Matrix{Cfloat}; id_offset::Union{Nothing,Integer}=nothing)
  d, n = size(X)
  d == ix.d || error("X must have d=$(ix.d) rows")
  id_offset = id_offset === nothing ? _ivf_next_id(ix) : id_offset
  _check(ccall((:rq_ivf_add, librayuela_hip), Cint, (Ptr{Cvoid}, Ptr{Cfloat}, Int64, UInt32),
               ix.h, X, Int64(n), UInt32(id_offset)))
  return ix
end

function add!(ix::HipIvfIndex, X::Matrix{UInt8}; id_offset::Union{Nothing,Integer}=nothing)
  d, n = size(X)
  d == ix.d || error("X must have d=$(ix.d) rows")
  id_offset = id_offset === nothing ? _ivf_next_id(ix) : id_offset
  _check(ccall((:rq_ivf_add_bytes, librayuela_hip), Cint, (Ptr{Cvoid}, Ptr{UInt8}, Int64, UInt32),
               ix.h, X, Int64(n), UInt32(id_offset)))
  return ix
end

function add_codes!(ix::HipIvfIndex, lists::Vector{UInt32}, B::Matrix{UInt8}; id_offset::Union{Nothing,Integer}=nothing)
  m, n = size(B)
  (m == ix.m && length(lists) == n) || error("codes must be m=$(ix.m) by n=$(length(lists))")
  id_offset = id_offset === nothing ? _ivf_next_id(ix) : id_offset
  _check(ccall((:rq_ivf_add_codes, librayuela_hip), Cint, (Ptr{Cvoid}, Ptr{UInt32}, Ptr{UInt8}, Int64, UInt32),
               ix.h, lists, B, Int64(n), UInt32(id_offset)))
  return ix
end

function search(ix::HipIvfIndex, X::Matrix{Cfloat}, nprobe::Int, k::Int)
  d, nq = size(X)
  d == ix.d || error("queries must have d=$(ix.d) rows")
  1 <= nprobe <= ix.nlist || error("1 <= nprobe <= nlist=$(ix.nlist); got $nprobe")
  dists = Matrix{Cfloat}(undef, k, nq)
  res   = Matrix{Cuint}(undef, k, nq)
  id_base = 1
  _check(ccall((:rq_ivf_search, librayuela_hip), Cint,
    (Ptr{Cvoid}, Ptr{Cfloat}, Ptr{Cuint}, Ptr{Cfloat}, Int64, Cint, Cint, Cint),
    ix.h, dists, res, X, Int64(nq), Cint(nprobe), Cint(k), Cint(id_base)))
  return dists, res
end

"""
    train_ivfpq(X, nlist, m; niter=25, seed=0, by_residual=true) -> Q, C
`Q` = the nlist centroids of `train_pq(X, 1, nlist)`; `C` = `train_pq` with 256 codewords on the residuals `x - Q[:, list(x)]`
(one stage of `quantize_rvq`, taken from rq_encode_rvq_wide), or on `X` itself without `by_residual`.
"""
function train_ivfpq(X::Matrix{Float32}, nlist::Integer, m::Integer; niter::Integer=25, seed::Integer=0, by_residual::Bool=true)
  d, n = size(X)
  Cq, _, _ = train_pq(X, 1, nlist, niter; seed=seed)
  Q = Cq[1]
  Xe = X
  if by_residual
    Xe = Matrix{Float32}(undef, d, n)
    B = Matrix{Int16}(undef, 1, n)
    h = nlist
    code_base = 1
    _check(ccall((:rq_encode_rvq_wide, librayuela_hip), Cint,
      (Ptr{Int16}, Ptr{Cfloat}, Ptr{Cfloat}, Int64, Cint, Cint, Cint, Cint, Ptr{UInt32}, Ptr{Cfloat}),
      B, X, Q, Int64(n), Cint(d), Cint(1), Cint(h), Cint(code_base), C_NULL, Xe))
  end
  C, _, _ = train_pq(Xe, m, 256, niter; seed=seed + 1)
  return Q, C
end

"""
    HipAqIndex(C; kind=:lsq, devices=nothing)
    HipAqIndexU16(C; kind=:lsq, devices=nothing)
The resident, row-sharded index of an additive quantizer: `C` holds m full-dimensional `d`-by-h codebooks (h = 256 for
`HipAqIndex`, any 1 <= h <= 32767 and m <= 32 for `HipAqIndexU16`); `kind` is `:lsq` (`linscan_lsq`) or `:cq` (`linscan_cq`).
`set_codes!(ix, B; dbnorms=..., cbnorms=...)` takes exactly one of the two for `:lsq` (with `cbnorms` the row norms are
quantized on the devices), neither for `:cq`; `search(ix, X, k; R=R)` returns what `linscan_lsq(B, X, C, dbnorms, R, k)` /
`linscan_cq(B, X, C, k)` return on the whole base (k-by-nq `dists`, ONE-based `idx`), bit for bit.
"""
mutable struct HipAqIndex
  h::Ptr{Cvoid}
  m::Int
  d::Int
  function HipAqIndex(C::Vector{Matrix{Cfloat}}; kind::Symbol=:lsq, devices::Union{Nothing,Vector{<:Integer}}=nothing)
    m = length(C)
    d = size(C[1], 1)
    lut_mode = _aq_lut_mode(kind)
    devs = devices === nothing ? Cint[] : convert(Vector{Cint}, devices)
    ptr = ccall((:rq_index_create_aq, librayuela_hip), Ptr{Cvoid}, (Cint, Cint, Ptr{Cfloat}, Cint, Ptr{Cint}, Cint),
                Cint(m), Cint(d), hcat(C...), Cint(lut_mode), devices === nothing ? C_NULL : devs, Cint(length(devs)))
    ptr == C_NULL && error("rq_index_create_aq: " * unsafe_string(ccall((:rq_last_error, librayuela_hip), Cstring, ())))
    ix = new(ptr, m, d)
    finalizer(x -> (x.h != C_NULL && ccall((:rq_index_destroy, librayuela_hip), Cvoid, (Ptr{Cvoid},), x.h); x.h = C_NULL), ix)
    return ix
  end
end

mutable struct HipAqIndexU16
  h::Ptr{Cvoid}
  m::Int
  d::Int
  function HipAqIndexU16(C::Vector{Matrix{Cfloat}}; kind::Symbol=:lsq, devices::Union{Nothing,Vector{<:Integer}}=nothing)
    m = length(C)
    d, h = size(C[1])
    lut_mode = _aq_lut_mode(kind)
    devs = devices === nothing ? Cint[] : convert(Vector{Cint}, devices)
    ptr = ccall((:rq_index_create_aq_wide, librayuela_hip), Ptr{Cvoid}, (Cint, Cint, Cint, Ptr{Cfloat}, Cint, Ptr{Cint}, Cint),
                Cint(m), Cint(h), Cint(d), hcat(C...), Cint(lut_mode), devices === nothing ? C_NULL : devs, Cint(length(devs)))
    ptr == C_NULL && error("rq_index_create_aq_wide: " * unsafe_string(ccall((:rq_last_error, librayuela_hip), Cstring, ())))
    ix = new(ptr, m, d)
    finalizer(x -> (x.h != C_NULL && ccall((:rq_index_destroy, librayuela_hip), Cvoid, (Ptr{Cvoid},), x.h); x.h = C_NULL), ix)
    return ix
  end
end

_aq_lut_mode(kind::Symbol) = kind === :lsq ? 1 : kind === :cq ? 2 : error("kind must be :lsq or :cq")
_aq_norm_ptr(v::Union{Nothing,Vector{Cfloat}}) = v === nothing ? Ptr{Cfloat}(C_NULL) : pointer(v)

function set_codes!(ix::HipAqIndex, B::Matrix{UInt8}; dbnorms::Union{Nothing,Vector{Cfloat}}=nothing,
                    cbnorms::Union{Nothing,Vector{Cfloat}}=nothing, id_offset::Integer=0)      # B zero-based m-by-n
  dbnorms === nothing || length(dbnorms) == size(B, 2) || error("dbnorms must have one entry per database row")
  hn = cbnorms === nothing ? 0 : length(cbnorms)
  GC.@preserve dbnorms cbnorms _check(ccall((:rq_index_set_codes_aq, librayuela_hip), Cint,
    (Ptr{Cvoid}, Ptr{Cuchar}, Ptr{Cfloat}, Ptr{Cfloat}, Cint, Int64, UInt32),
    ix.h, B, _aq_norm_ptr(dbnorms), _aq_norm_ptr(cbnorms), Cint(hn), Int64(size(B, 2)), UInt32(id_offset)))
  return ix
end
set_codes!(ix::HipAqIndex, B::Matrix{T}; kwargs...) where T <: Integer = set_codes!(ix, convert(Matrix{UInt8}, B .- 1); kwargs...)

function set_codes!(ix::HipAqIndexU16, B::Matrix{Int16}; dbnorms::Union{Nothing,Vector{Cfloat}}=nothing,
                    cbnorms::Union{Nothing,Vector{Cfloat}}=nothing, code_base::Integer=0, id_offset::Integer=0)
  dbnorms === nothing || length(dbnorms) == size(B, 2) || error("dbnorms must have one entry per database row")
  hn = cbnorms === nothing ? 0 : length(cbnorms)
  GC.@preserve dbnorms cbnorms _check(ccall((:rq_index_set_codes_aq_wide, librayuela_hip), Cint,
    (Ptr{Cvoid}, Ptr{Int16}, Ptr{Cfloat}, Ptr{Cfloat}, Cint, Int64, Cint, UInt32),
    ix.h, B, _aq_norm_ptr(dbnorms), _aq_norm_ptr(cbnorms), Cint(hn), Int64(size(B, 2)), Cint(code_base), UInt32(id_offset)))
  return ix
end
set_codes!(ix::HipAqIndexU16, B::Matrix{T}; kwargs...) where T <: Integer =
  set_codes!(ix, convert(Matrix{Int16}, B); code_base=1, kwargs...)

search(ix::Union{HipAqIndex,HipAqIndexU16}, X::Matrix{Cfloat}, k::Int=10000; R::Union{Nothing,Matrix{Cfloat}}=nothing) =
  _index_search(ix, X, k, R)

"""
    HipDataset(X)
`X` (d-by-n) uploaded once; `quantize(ds, C)` == `quantize_pq(X, C)`, `quantize(ds, C; R=R)` == `quantize_opq(X, R, C)`.
`X::Matrix{UInt8}` (bvecs data) stays bytes on the device.  Codebooks of more than 256 codewords take rq_dataset_encode_wide.
"""
mutable struct HipDataset
  h::Ptr{Cvoid}
  n::Int
  function HipDataset(X::Matrix{Float32})
    d, n = size(X)
    h = ccall((:rq_dataset_upload, librayuela_hip), Ptr{Cvoid}, (Ptr{Cfloat}, Int64, Cint), X, Int64(n), Cint(d))
    h == C_NULL && error("rq_dataset_upload: " * unsafe_string(ccall((:rq_last_error, librayuela_hip), Cstring, ())))
    ds = new(h, n)
    finalizer(x -> (x.h != C_NULL && ccall((:rq_dataset_free, librayuela_hip), Cvoid, (Ptr{Cvoid},), x.h); x.h = C_NULL), ds)
    return ds
  end
  function HipDataset(X::Matrix{UInt8})
    d, n = size(X)
    h = ccall((:rq_dataset_upload_bytes, librayuela_hip), Ptr{Cvoid}, (Ptr{UInt8}, Int64, Cint), X, Int64(n), Cint(d))
    h == C_NULL && error("rq_dataset_upload_bytes: " * unsafe_string(ccall((:rq_last_error, librayuela_hip), Cstring, ())))
    ds = new(h, n)
    finalizer(x -> (x.h != C_NULL && ccall((:rq_dataset_free, librayuela_hip), Cvoid, (Ptr{Cvoid},), x.h); x.h = C_NULL), ds)
    return ds
  end
end

function quantize(ds::HipDataset, C::Vector{Matrix{Float32}}; R::Union{Nothing,Matrix{Float32}}=nothing)
  m, h = length(C), size(C[1], 2)
  B = Matrix{Int16}(undef, m, ds.n)
  if h > 256
    code_base = 1
    _check(ccall((:rq_dataset_encode_wide, librayuela_hip), Cint,
      (Ptr{Cvoid}, Ptr{Int16}, Ptr{Cfloat}, Ptr{Cfloat}, Cint, Cint, Cint),
      ds.h, B, R === nothing ? C_NULL : R, _cat_codebooks(C), Cint(m), Cint(h), Cint(code_base)))
    return B
  end
  _check(ccall((:rq_dataset_encode, librayuela_hip), Cint,
    (Ptr{Cvoid}, Ptr{Cuchar}, Ptr{Int16}, Ptr{Cfloat}, Ptr{Cfloat}, Cint, Cint),
    ds.h, C_NULL, B, R === nothing ? C_NULL : R, _cat_codebooks(C), Cint(m), Cint(h)))
  return B
end

"""
    rerank(ds, X, cand, k; id_offset=0) -> dists, ids
The candidates of a search (`cand`, kc-by-nq ONE-based `UInt32` ids as `search` returns them) ordered by their exact Float32
distance to the rows of the resident `ds`: the `k` nearest per query, k-by-nq.  Column i of the uploaded matrix has id
`i + id_offset`.  Ids outside the base (the searches' padding id among them) are skipped, an id given twice appears twice, and
a short list ends in the padding pair (rq_dataset_rerank).
"""
function rerank(ds::HipDataset, X::Matrix{Cfloat}, cand::Matrix{UInt32}, k::Integer; id_offset::Integer=0)
  kc, nq = size(cand)
  size(X, 2) == nq || error("one column of candidates per query")
  1 <= k <= kc || error("1 <= k <= kc=$kc; got $k")
  dists = Matrix{Cfloat}(undef, k, nq)
  res   = Matrix{Cuint}(undef, k, nq)
  ldc = kc
  id_base = 1
  _check(ccall((:rq_dataset_rerank, librayuela_hip), Cint,
    (Ptr{Cvoid}, Ptr{Cfloat}, Ptr{Cuint}, Ptr{Cfloat}, Int64, Ptr{Cuint}, Int64, Int64, Cint, UInt32, Cint),
    ds.h, dists, res, X, Int64(nq), cand, Int64(kc), Int64(ldc), Cint(k), UInt32(id_offset), Cint(id_base)))
  return dists, res
end

"""
    search_refine(ix, ds, X, nprobe, k, kc; id_offset=0)    # HipIvfIndex: on the device, no host round trip
    search_refine(ix, ds, X, k, kc; R=nothing)               # HipIndex / HipIndexU16 / HipAqIndex / HipAqIndexU16
`search` with `kc` candidates per query, re-ranked by `rerank(ds, X, cand, k)`: bit for bit that composition.  The queries are
re-ranked unrotated against the unrotated base.
"""
function search_refine(ix::HipIvfIndex, ds::HipDataset, X::Matrix{Cfloat}, nprobe::Int, k::Int, kc::Int; id_offset::Integer=0)
  d, nq = size(X)
  d == ix.d || error("queries must have d=$(ix.d) rows")
  1 <= nprobe <= ix.nlist || error("1 <= nprobe <= nlist=$(ix.nlist); got $nprobe")
  1 <= k <= kc || error("1 <= k <= kc=$kc; got $k")
  dists = Matrix{Cfloat}(undef, k, nq)
  res   = Matrix{Cuint}(undef, k, nq)
  id_base = 1
  _check(ccall((:rq_ivf_search_refine, librayuela_hip), Cint,
    (Ptr{Cvoid}, Ptr{Cvoid}, Ptr{Cfloat}, Ptr{Cuint}, Ptr{Cfloat}, Int64, Cint, Cint, Cint, UInt32, Cint),
    ix.h, ds.h, dists, res, X, Int64(nq), Cint(nprobe), Cint(k), Cint(kc), UInt32(id_offset), Cint(id_base)))
  return dists, res
end

function search_refine(ix::Union{HipIndex,HipIndexU16,HipAqIndex,HipAqIndexU16}, ds::HipDataset, X::Matrix{Cfloat}, k::Int, kc::Int;
                       R::Union{Nothing,Matrix{Cfloat}}=nothing)
  _, cand = R === nothing ? search(ix, X, kc) : search(ix, X, kc; R=R)
  return rerank(ds, X, convert(Matrix{UInt32}, cand), k)
end

# ---- LSQ encoding (src/LSQ.jl:272-302, src/LSQ_GPU.jl:218-264): ILS around ICM on the device (rq_encode_icm) ----------
# Codes are Int16 one-based m x n like the reference; the random stream is counter-based (`seed`), so results depend on
# neither nsplits nor checkpoints (DESIGN.md section 2).
function _encode_icm!(out::Matrix{UInt8}, B0::Matrix{UInt8}, cost, X::Matrix{Float32}, C::Vector{Matrix{Float32}},
                      ilsiter, icmiter, npert, randord, seed, t0, nsplits)
  d, n = size(X)
  m    = length(C)
  h    = size(C[1], 2)
  _check(ccall((:rq_encode_icm, librayuela_hip), Cint,
    (Ptr{UInt8}, Ptr{UInt8}, Ptr{Cfloat}, Ptr{Cfloat}, Ptr{Cfloat}, Int64, Cint, Cint, Cint, Cint, Cint, Cint, Cint,
     UInt64, Int64, Cint),
    out, B0, cost === nothing ? C_NULL : cost, X, hcat(C...), Int64(n), Cint(d), Cint(m), Cint(h), Cint(ilsiter),
    Cint(icmiter), Cint(npert), Cint(randord ? 1 : 0), UInt64(seed), Int64(t0), Cint(nsplits)))
  return out
end

# More than 256 codewords per codebook (rq_encode_icm_wide, DESIGN.md section 4.24): the same contract over the reference's own
# one-based Int16 codes, up to h = 32767 where the pair tables fit the scratch budget (icm_wide_plan says so without a device).
function _encode_icm_wide!(out::Matrix{Int16}, B0::Matrix{Int16}, cost, X::Matrix{Float32}, C::Vector{Matrix{Float32}},
                           ilsiter, icmiter, npert, randord, seed, t0, nsplits)
  d, n = size(X)
  m    = length(C)
  h    = size(C[1], 2)
  code_base = 1
  _check(ccall((:rq_encode_icm_wide, librayuela_hip), Cint,
    (Ptr{Int16}, Ptr{Int16}, Ptr{Cfloat}, Ptr{Cfloat}, Ptr{Cfloat}, Int64, Cint, Cint, Cint, Cint, Cint, Cint, Cint,
     UInt64, Int64, Cint, Cint),
    out, B0, cost === nothing ? C_NULL : cost, X, hcat(C...), Int64(n), Cint(d), Cint(m), Cint(h), Cint(ilsiter),
    Cint(icmiter), Cint(npert), Cint(randord ? 1 : 0), UInt64(seed), Int64(t0), Cint(nsplits), Cint(code_base)))
  return out
end

# (HS, bytes of the tables, bytes of one row's unaries, rows per chunk, chunks) of an encode at h > 256; throws where it would
function icm_wide_plan(n::Integer, d::Integer, m::Integer, h::Integer, nsplits::Integer=1)
  out = Vector{Int64}(undef, 5)
  cap = length(out)
  _check(ccall((:rq_icm_wide_plan, librayuela_hip), Cint, (Int64, Cint, Cint, Cint, Cint, Ptr{Int64}, Cint),
    Int64(n), Cint(d), Cint(m), Cint(h), Cint(nsplits), out, Cint(cap)))
  return out
end

function encoding_icm(X::Matrix{Float32}, oldB::Matrix{Int16}, C::Vector{Matrix{Float32}}, ilsiter::Integer,
                      icmiter::Integer, randord::Bool, npert::Integer, cpp::Bool=true, V::Bool=false; seed::Integer=0)
  h = size(C[1], 2)
  cpp && h != 256 && throw(ArgumentError("encoding_icm with cpp=true requires h = 256 codewords; got h=$h"))
  if h > 256
    B = _encode_icm_wide!(similar(oldB), oldB, nothing, X, C, ilsiter, icmiter, npert, randord, seed, 0, 1)
    copyto!(oldB, B)
    return B
  end
  B0  = convert(Matrix{UInt8}, oldB .- Int16(1))
  out = similar(B0)
  _encode_icm!(out, B0, nothing, X, C, ilsiter, icmiter, npert, randord, seed, 0, 1)
  B = convert(Matrix{Int16}, out) .+ Int16(1)
  copyto!(oldB, B)
  return B
end

function encode_icm_cuda(RX::Matrix{Float32}, B::Matrix{Int16}, C::Vector{Matrix{Float32}}, ilsiters::Vector{Int64},
                         icmiter::Integer, npert::Integer, randord::Bool, nsplits::Integer=2, V::Bool=false;
                         seed::Integer=0)
  wide = size(C[1], 2) > 256
  cur  = wide ? copy(B) : convert(Matrix{UInt8}, B .- Int16(1))
  cost = Vector{Float32}(undef, size(RX, 2))
  Bs   = Vector{Matrix{Int16}}(undef, length(ilsiters))
  objs = zeros(Float32, length(ilsiters))
  done = 0
  for stop in sort(unique(ilsiters))
    nxt = similar(cur)
    if wide
      _encode_icm_wide!(nxt, cur, cost, RX, C, stop - done, icmiter, npert, randord, seed, done, nsplits)
    else
      _encode_icm!(nxt, cur, cost, RX, C, stop - done, icmiter, npert, randord, seed, done, nsplits)
    end
    cur, done = nxt, stop
    for (i, s) in enumerate(ilsiters)
      if s == stop
        Bs[i]   = wide ? copy(cur) : convert(Matrix{Int16}, cur) .+ Int16(1)
        objs[i] = Float32(sum(Float64.(cost)) / length(cost))
      end
    end
    V && println(" ILS iteration $stop/$(maximum(ilsiters)) done")
  end
  return Bs, objs
end

# ---- LSQ codebook update (src/codebook_update.jl:175-206, :235-277) and training (src/LSQ.jl:323-372,
# src/LSQ_GPU.jl:267-319): the normal equations and their f64 solve run on the device (DESIGN.md section 2) ----------
_split_codebooks(Cc::Matrix{Float32}, m, h) = [Cc[:, (i - 1) * h + 1:i * h] for i = 1:m]

function update_codebooks_fast_bin(X::Matrix{Float32}, B::Matrix{Int16}, h::Integer, V::Bool=false, rho::Float64=1e-4)
  d, n  = size(X)
  m     = size(B, 1)
  codes = convert(Matrix{UInt8}, B .- Int16(1))
  Cc    = Matrix{Float32}(undef, d, m * h)
  _check(ccall((:rq_update_codebooks_lsq, librayuela_hip), Cint,
    (Ptr{Cfloat}, Ptr{Cfloat}, Ptr{UInt8}, Int64, Cint, Cint, Cint, Cdouble),
    Cc, X, codes, Int64(n), Cint(d), Cint(m), Cint(h), Float64(rho)))
  V && println("Doing fast bin codebook update... done.")
  return _split_codebooks(Cc, m, h)
end

# More than 256 codewords per codebook (rq_update_codebooks_lsq_wide, DESIGN.md section 4.25): the same contract over the
# reference's own one-based Int16 codes, up to h = 32767 with m * h <= 16384 (lsq_wide_plan says so without a device).
function _update_codebooks_wide(X::Matrix{Float32}, B::Matrix{Int16}, h::Integer, rho::Float64=1e-4)
  d, n  = size(X)
  m     = size(B, 1)
  Cc    = Matrix{Float32}(undef, d, m * h)
  code_base = 1
  _check(ccall((:rq_update_codebooks_lsq_wide, librayuela_hip), Cint,
    (Ptr{Cfloat}, Ptr{Cfloat}, Ptr{Int16}, Int64, Cint, Cint, Cint, Cdouble, Cint),
    Cc, X, B, Int64(n), Cint(d), Cint(m), Cint(h), Float64(rho), Cint(code_base)))
  return _split_codebooks(Cc, m, h)
end

# fast_bin_matmul's A (mh x mh) and b (memory image [mh][d]: a d x mh matrix here) and the rows per (codebook, code) at any
# h <= 32767 (rq_lsq_normal_eq_wide); with_A = false: b and the counts alone, for shapes past m * h = 16384
function lsq_normal_eq_wide(X::Matrix{Float32}, B::Matrix{Int16}, h::Integer; rho::Float64=1e-4, with_A::Bool=true)
  d, n   = size(X)
  m      = size(B, 1)
  A      = with_A ? Matrix{Float64}(undef, m * h, m * h) : nothing
  b      = Matrix{Float64}(undef, d, m * h)
  counts = Matrix{UInt32}(undef, h, m)
  code_base = 1
  _check(ccall((:rq_lsq_normal_eq_wide, librayuela_hip), Cint,
    (Ptr{Cdouble}, Ptr{Cdouble}, Ptr{UInt32}, Ptr{Cfloat}, Ptr{Int16}, Int64, Cint, Cint, Cint, Cdouble, Cint),
    A === nothing ? C_NULL : A, b, counts, X, B, Int64(n), Cint(d), Cint(m), Cint(h), Float64(rho), Cint(code_base)))
  return A, b, counts
end

# (m*h, bytes of A, bytes of the pair counts, bytes of the sort scratch, tiles, Cholesky block steps, train_lsq can run it) of an
# update at h > 256; throws where rq_update_codebooks_lsq_wide would
function lsq_wide_plan(n::Integer, d::Integer, m::Integer, h::Integer)
  out = Vector{Int64}(undef, 7)
  cap = length(out)
  _check(ccall((:rq_lsq_wide_plan, librayuela_hip), Cint, (Int64, Cint, Cint, Cint, Ptr{Int64}, Cint),
    Int64(n), Cint(d), Cint(m), Cint(h), out, Cint(cap)))
  return out
end

function update_codebooks(X::Matrix{Float32}, B::Matrix{Int16}, h::Integer, V::Bool=false,
                          method::AbstractString="fastbin")
  method in ["fast", "fastbin", "lsmr", "lsqr", "naive"] || error("Codebook update method unknown")
  method == "fastbin" || throw(ArgumentError("codebook update method \"$method\" is not supported; only \"fastbin\" is"))
  h > 256 || return update_codebooks_fast_bin(X, B, h, V)
  C = _update_codebooks_wide(X, B, h)
  V && println("Doing fast bin codebook update... done.")
  return C
end

function _train_lsq_wide(X::Matrix{Float32}, m, h, R::Matrix{Float32}, B::Matrix{Int16}, niter, ilsiter, icmiter, randord,
                         npert, seed, nsplits)
  d, n  = size(X)
  codes = copy(B)
  Cc    = Matrix{Float32}(undef, d, m * h)
  obj   = zeros(Float64, max(niter, 1))
  code_base = 1
  _check(ccall((:rq_train_lsq_wide, librayuela_hip), Cint,
    (Ptr{Cfloat}, Ptr{Int16}, Ptr{Cdouble}, Ptr{Cfloat}, Ptr{Cfloat}, Int64, Cint, Cint, Cint, Cint, Cint, Cint, Cint,
     Cint, UInt64, Cint, Cint),
    Cc, codes, obj, X, R, Int64(n), Cint(d), Cint(m), Cint(h), Cint(niter), Cint(ilsiter), Cint(icmiter), Cint(npert),
    Cint(randord ? 1 : 0), UInt64(seed), Cint(nsplits), Cint(code_base)))
  return _split_codebooks(Cc, m, h), codes, convert(Vector{Float32}, obj[1:niter])
end

function _train_lsq(X::Matrix{Float32}, m, h, R::Matrix{Float32}, B::Matrix{Int16}, niter, ilsiter, icmiter, randord,
                    npert, seed, nsplits)
  h > 256 && return _train_lsq_wide(X, m, h, R, B, niter, ilsiter, icmiter, randord, npert, seed, nsplits)
  d, n  = size(X)
  codes = convert(Matrix{UInt8}, B .- Int16(1))
  Cc    = Matrix{Float32}(undef, d, m * h)
  obj   = zeros(Float64, max(niter, 1))
  _check(ccall((:rq_train_lsq, librayuela_hip), Cint,
    (Ptr{Cfloat}, Ptr{UInt8}, Ptr{Cdouble}, Ptr{Cfloat}, Ptr{Cfloat}, Int64, Cint, Cint, Cint, Cint, Cint, Cint, Cint,
     Cint, UInt64, Cint),
    Cc, codes, obj, X, R, Int64(n), Cint(d), Cint(m), Cint(h), Cint(niter), Cint(ilsiter), Cint(icmiter), Cint(npert),
    Cint(randord ? 1 : 0), UInt64(seed), Cint(nsplits)))
  return _split_codebooks(Cc, m, h), convert(Matrix{Int16}, codes) .+ Int16(1), convert(Vector{Float32}, obj[1:niter])
end

function train_lsq(X::Matrix{Float32}, m::Integer, h::Integer, R::Matrix{Float32}, B::Matrix{Int16},
                   C::Vector{Matrix{Float32}}, niter::Integer, ilsiter::Integer, icmiter::Integer, randord::Bool,
                   npert::Integer, cpp::Bool=true, V::Bool=true; seed::Integer=0)
  cpp && h != 256 && throw(ArgumentError("train_lsq with cpp=true requires h = 256 codewords; got h=$h"))
  Cn, Bn, obj = _train_lsq(X, m, h, R, B, niter, ilsiter, icmiter, randord, npert, seed, 1)
  copyto!(B, Bn)          # the final codes land in B, as encoding_icm's do
  V && for (it, o) in enumerate(obj); println("$it $o"); end
  return Cn, Bn, obj
end

function train_lsq_cuda(X::Matrix{Float32}, m::Integer, h::Integer, R::Matrix{Float32}, B::Matrix{Int16},
                        C::Vector{Matrix{Float32}}, niter::Integer, ilsiter::Integer, icmiter::Integer, randord::Bool,
                        npert::Integer, nsplits::Integer=1, V::Bool=false; seed::Integer=0)
  Cn, Bn, obj = _train_lsq(X, m, h, R, B, niter, ilsiter, icmiter, randord, npert, seed, nsplits)
  V && for (it, o) in enumerate(obj); println("$it $o"); end
  return Cn, Bn, obj
end

# ---- LSQ++ (src/SR.jl:4-84, :88-176; src/SR_perturbations.jl:4-73): the noise (a counter-based standard normal variate,
# DESIGN.md section 2 "SR noise") and the training loop run on the device.  These shims follow the LSQ ones above and,
# like them, have not been run (no Julia was available).
function _sr_kind(method::AbstractString)
  method in ["SR_C", "SR_D"] || error("SR method unknown")
  return method == "SR_C" ? 0 : 1
end

function _sr_scale(iter::Integer, niter::Integer, schedule::Integer, p::AbstractFloat)
  scale = Ref{Cdouble}(0.0)
  _check(ccall((:rq_sr_schedule, librayuela_hip), Cint, (Ref{Cdouble}, Cint, Int64, Int64, Cdouble),
    scale, Cint(schedule), Int64(iter), Int64(niter), Float64(p)))
  return scale[]
end

function _sr_std(X::Matrix{Float32})
  d, n  = size(X)
  sigma = Vector{Float32}(undef, d)
  _check(ccall((:rq_sr_std, librayuela_hip), Cint, (Ptr{Cfloat}, Ptr{Cfloat}, Int64, Cint), sigma, X, Int64(n), Cint(d)))
  return sigma
end

function _sr_perturb(X::Matrix{Float32}, sigma::Vector{Float32}, scale::Float64, kind::Integer, seed::Integer,
                     call::Integer, row0::Integer=0)
  d, n = size(X)
  Y    = Matrix{Float32}(undef, d, n)
  _check(ccall((:rq_sr_perturb, librayuela_hip), Cint,
    (Ptr{Cfloat}, Ptr{Cfloat}, Ptr{Cfloat}, Cdouble, Int64, Cint, Cint, UInt64, Int64, Int64),
    Y, X, sigma, Float64(scale), Int64(n), Cint(d), Cint(kind), UInt64(seed), Int64(call), Int64(row0)))
  return Y
end

function SR_C_perturb(X::Matrix{Float32}, iter::Integer, niter::Integer, schedule::Integer=1, p::AbstractFloat=0.5;
                      seed::Integer=0, call::Integer=iter)
  return _sr_perturb(X, _sr_std(X), _sr_scale(iter, niter, schedule, p), 0, seed, call)
end

function SR_D_perturb(C::Vector{Matrix{Float32}}, iter::Integer, niter::Integer, schedule::Integer=1,
                      p::AbstractFloat=0.5; seed::Integer=0, call::Integer=iter)
  m     = length(C)
  h     = size(C[1], 2)
  Cc    = cat(C..., dims=2)
  sigma = _sr_std(Cc) ./ Float32(m)
  Y     = _sr_perturb(Cc, sigma, _sr_scale(iter, niter, schedule, p), 1, seed, call)
  for i = 1:m; C[i] .= Y[:, (i - 1) * h + 1:i * h]; end
  return C
end

# Past 256 codewords per codebook the loop runs over 16-bit codes (rq_train_sr_wide, DESIGN.md section 4.27): B goes in and comes
# back one-based (code_base = 1); flags = 0 leaves out the codebook updates that would repeat work (the same bits either way).
function _train_sr_wide(X::Matrix{Float32}, m, h, R::Matrix{Float32}, B::Matrix{Int16}, niter, ilsiter, icmiter, randord,
                        npert, method, schedule, p, clean_update, seed, nsplits)
  d, n  = size(X)
  codes = copy(B)
  Cc    = Matrix{Float32}(undef, d, m * h)
  obj   = zeros(Float64, niter + 1)
  code_base = 1
  flags = 0
  _check(ccall((:rq_train_sr_wide, librayuela_hip), Cint,
    (Ptr{Cfloat}, Ptr{Int16}, Ptr{Cdouble}, Ptr{Cfloat}, Ptr{Cfloat}, Int64, Cint, Cint, Cint, Cint, Cint, Cint, Cint,
     Cint, Cint, Cint, Cdouble, Cint, UInt64, Cint, Cint, Cint),
    Cc, codes, obj, X, R, Int64(n), Cint(d), Cint(m), Cint(h), Cint(niter), Cint(ilsiter), Cint(icmiter), Cint(npert),
    Cint(randord ? 1 : 0), Cint(_sr_kind(method)), Cint(schedule), Float64(p), Cint(clean_update ? 1 : 0), UInt64(seed),
    Cint(nsplits), Cint(code_base), Cint(flags)))
  return _split_codebooks(Cc, m, h), codes, convert(Vector{Float32}, obj)
end

function _train_sr(X::Matrix{Float32}, m, h, R::Matrix{Float32}, B::Matrix{Int16}, niter, ilsiter, icmiter, randord,
                   npert, method, schedule, p, clean_update, seed, nsplits)
  h > 256 && return _train_sr_wide(X, m, h, R, B, niter, ilsiter, icmiter, randord, npert, method, schedule, p, clean_update,
                                   seed, nsplits)
  d, n  = size(X)
  codes = convert(Matrix{UInt8}, B .- Int16(1))
  Cc    = Matrix{Float32}(undef, d, m * h)
  obj   = zeros(Float64, niter + 1)
  _check(ccall((:rq_train_sr, librayuela_hip), Cint,
    (Ptr{Cfloat}, Ptr{UInt8}, Ptr{Cdouble}, Ptr{Cfloat}, Ptr{Cfloat}, Int64, Cint, Cint, Cint, Cint, Cint, Cint, Cint,
     Cint, Cint, Cint, Cdouble, Cint, UInt64, Cint),
    Cc, codes, obj, X, R, Int64(n), Cint(d), Cint(m), Cint(h), Cint(niter), Cint(ilsiter), Cint(icmiter), Cint(npert),
    Cint(randord ? 1 : 0), Cint(_sr_kind(method)), Cint(schedule), Float64(p), Cint(clean_update ? 1 : 0), UInt64(seed),
    Cint(nsplits)))
  return _split_codebooks(Cc, m, h), convert(Matrix{Int16}, codes) .+ Int16(1), convert(Vector{Float32}, obj)
end

# As committed the reference passes p where the schedule is expected (src/SR.jl:35, :66); its evident intent, schedule 1
# with power p, runs here.  No codebook update follows an iteration's encode.
function train_sr(X::Matrix{Float32}, m::Integer, h::Integer, R::Matrix{Float32}, B::Matrix{Int16},
                  C::Vector{Matrix{Float32}}, niter::Integer, ilsiter::Integer, icmiter::Integer, randord::Bool,
                  npert::Integer, method::AbstractString, p::Float32, cpp::Bool=true, V::Bool=false; seed::Integer=0)
  cpp && h != 256 && throw(ArgumentError("train_sr with cpp=true requires h = 256 codewords; got h=$h"))
  Cn, Bn, obj = _train_sr(X, m, h, R, B, niter, ilsiter, icmiter, randord, npert, method, 1, p, false, seed, 1)
  copyto!(B, Bn)          # the final codes land in B, as encoding_icm's do
  V && for (it, o) in enumerate(obj); println("$it $o"); end
  return Cn, Bn, obj
end

function train_sr_cuda(X::Matrix{Float32}, m::Integer, h::Integer, R::Matrix{Float32}, B::Matrix{Int16},
                       C::Vector{Matrix{Float32}}, niter::Integer, ilsiter::Integer, icmiter::Integer, randord::Bool,
                       npert::Integer, method::AbstractString, schedule::Integer, p::AbstractFloat=0.5,
                       nsplits::Integer=1, V::Bool=false; seed::Integer=0)
  Cn, Bn, obj = _train_sr(X, m, h, R, B, niter, ilsiter, icmiter, randord, npert, method, schedule, p, true, seed,
                          nsplits)
  V && for (it, o) in enumerate(obj); println("$it $o"); end
  return Cn, Bn, obj
end

# ---- Chain quantization (src/ChainQ.jl:305-348, :373-431; src/codebook_update.jl:280-294, :367-412): the Viterbi
# recursion, the chain-structured codebook update and the training loop run on the device (DESIGN.md section 2).  These
# shims follow the LSQ ones above and, like them, have not been run (no Julia was available).  Past 256 codewords per codebook
# they call the entries over Int16 codes (DESIGN.md section 4.26) with code_base = 1: Julia's own one-based codes go in and out.
function quantize_chainq(X::Matrix{Float32}, C::Vector{Matrix{Float32}}, use_cuda::Bool=false, use_cpp::Bool=false)
  start_time = time_ns()
  d, n  = size(X)
  m     = length(C)
  h     = size(C[1], 2)
  if h > 256
    B = Matrix{Int16}(undef, m, n)
    _check(ccall((:rq_quantize_chainq_wide, librayuela_hip), Cint,
      (Ptr{Int16}, Ptr{Cfloat}, Ptr{Cfloat}, Int64, Cint, Cint, Cint, Cint, Cint),
      B, X, hcat(C...), Int64(n), Cint(d), Cint(m), Cint(h), Cint(1), Cint(1)))
    return B, (time_ns() - start_time) / 1e9
  end
  codes = Matrix{UInt8}(undef, m, n)
  _check(ccall((:rq_quantize_chainq, librayuela_hip), Cint,
    (Ptr{UInt8}, Ptr{Cfloat}, Ptr{Cfloat}, Int64, Cint, Cint, Cint, Cint),
    codes, X, hcat(C...), Int64(n), Cint(d), Cint(m), Cint(h), Cint(1)))
  return convert(Matrix{Int16}, codes) .+ Int16(1), (time_ns() - start_time) / 1e9
end

function get_cbdims_chain(d::Integer, m::Integer)
  lo = Vector{Cint}(undef, m)
  hi = Vector{Cint}(undef, m)
  _check(ccall((:rq_chain_dims, librayuela_hip), Cint, (Cint, Cint, Ptr{Cint}, Ptr{Cint}), Cint(d), Cint(m), lo, hi))
  return [Int(lo[i]) + 1:Int(hi[i]) for i = 1:m]
end

function update_codebooks_chain_bin(X::Matrix{Float32}, B::Matrix{Int16}, h::Integer, V::Bool=false, rho::Float64=1e-4)
  start_time = time_ns()
  d, n  = size(X)
  m     = size(B, 1)
  Cc    = Matrix{Float32}(undef, d, m * h)
  if h > 256
    _check(ccall((:rq_update_codebooks_chain_wide, librayuela_hip), Cint,
      (Ptr{Cfloat}, Ptr{Cfloat}, Ptr{Int16}, Int64, Cint, Cint, Cint, Cdouble, Cint),
      Cc, X, B, Int64(n), Cint(d), Cint(m), Cint(h), Float64(rho), Cint(1)))
    return _split_codebooks(Cc, m, h), (time_ns() - start_time) / 1e9
  end
  codes = convert(Matrix{UInt8}, B .- Int16(1))
  _check(ccall((:rq_update_codebooks_chain, librayuela_hip), Cint,
    (Ptr{Cfloat}, Ptr{Cfloat}, Ptr{UInt8}, Int64, Cint, Cint, Cint, Cdouble),
    Cc, X, codes, Int64(n), Cint(d), Cint(m), Cint(h), Float64(rho)))
  return _split_codebooks(Cc, m, h), (time_ns() - start_time) / 1e9
end

function train_chainq(X::Matrix{Float32}, m::Integer, h::Integer, R::Matrix{Float32}, B::Matrix{Int16},
                      C::Vector{Matrix{Float32}}, niter::Integer, V::Bool=false)
  V && println("Training a chain quantizer")
  d, n  = size(X)
  Cc    = Matrix{Float32}(undef, d, m * h)
  Rn    = copy(R)
  obj   = zeros(Float64, niter + 1)
  if h > 256
    Bn = copy(B)
    _check(ccall((:rq_train_chainq_wide, librayuela_hip), Cint,
      (Ptr{Cfloat}, Ptr{Int16}, Ptr{Cfloat}, Ptr{Cdouble}, Ptr{Cfloat}, Int64, Cint, Cint, Cint, Cint, Cint),
      Cc, Bn, Rn, obj, X, Int64(n), Cint(d), Cint(m), Cint(h), Cint(niter), Cint(1)))
    V && for (it, o) in enumerate(obj); println("$(it - 1) $o"); end
    return _split_codebooks(Cc, m, h), Bn, Rn, convert(Vector{Float32}, obj)
  end
  codes = convert(Matrix{UInt8}, B .- Int16(1))
  _check(ccall((:rq_train_chainq, librayuela_hip), Cint,
    (Ptr{Cfloat}, Ptr{UInt8}, Ptr{Cfloat}, Ptr{Cdouble}, Ptr{Cfloat}, Int64, Cint, Cint, Cint, Cint),
    Cc, codes, Rn, obj, X, Int64(n), Cint(d), Cint(m), Cint(h), Cint(niter)))
  V && for (it, o) in enumerate(obj); println("$(it - 1) $o"); end
  return _split_codebooks(Cc, m, h), convert(Matrix{Int16}, codes) .+ Int16(1), Rn, convert(Vector{Float32}, obj)
end

# Diagnostics: the kept in-call row order of raw-pointer scans on the current device since the last release
# (include/rayuela_hip.h, rq_order_cache_stats): consulted, hits, plain builds, balanced builds, uncached, upgrades.
function order_cache_stats()
  out8 = zeros(UInt64, 8)
  _check(ccall((:rq_order_cache_stats, librayuela_hip), Cint, (Ptr{UInt64},), out8))
  return (consulted=out8[1], hits=out8[2], plain_builds=out8[3], balanced_builds=out8[4], uncached=out8[5], upgrades=out8[6])
end

end # module
