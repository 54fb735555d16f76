// param_amd/csrc/bwd_sorted_apply_impl.inc -- destination element types, kernels and launchers of the sorted backward's
// apply; included once by each embbag_bwd_sorted_<dtype>.hip (inside namespace pm::{anonymous}).
// ---------------------------------------------------------------------------------------------
// step 3 helpers: destination element types
// 16-byte destination-row accesses; nt = streaming hint (every touched row is read once and written
// once per call, so it should not displace the gradient rows that ARE re-read from L2)
// cache policy of the destination-row accesses (SortedParams::nt_rows, pm_set_tuning nt_loads): 0 default, 1 non-temporal
// (nt), 2 system scope (volatile: sc0 sc1 -- misses the non-coherent caches on the way in, writes through on the way out)
// 3 / 4: plain / non-temporal load, agent-scope (sc1) store -- the store writes through and DROPS the line from the XCD's L2
// (MI355X_MICROARCH.md, store flavours), so a row occupies L2 only between its load and its store and the re-read gradient
// rows keep the capacity
__device__ __forceinline__ u32x4 raw16_load(const char* p, int pol) {
    const PM_GLOBAL u32x4* q = as_global<u32x4>(p);   // global, not flat (common.h)
    if (pol == 2) return *reinterpret_cast<const volatile PM_GLOBAL u32x4*>(q);
    return (pol == 1 || pol == 4) ? __builtin_nontemporal_load(q) : *q;
}
// Every store of the apply kernels is inline assembly, so that the compiler's wait-count bookkeeping sees LOADS only: on gfx9
// stores count in vmcnt too and return out of order with respect to loads, and with a store it knows of still pending the
// compiler waits for a load with `s_waitcnt vmcnt(0)` -- for every access outstanding, the write-through row stores included.
// That wait stood in front of EVERY position of the main kernel's batch: one position's loads in flight at a time, each
// waiting for the row stores before it.  With the stores out of its sight the waits are counted (vmcnt(N)); a count can only
// come out too high for the hardware (over-waiting), never too low: a load is older than the N loads issued after it, those
// cannot complete before it, so while it is pending more than N accesses are.  `s_nop 1`: the data registers of a wide store
// must not be overwritten by the next instruction (the hazard the compiler pads for its own stores).
// -DPM_VISIBLE_STORES rebuilds every store of these kernels as a plain, compiler-visible store (the compiler then orders its
// waits itself: slower, one position's loads in flight again, and independent of the assumption the hidden stores lean on --
// that on gfx950 a wave's vector-memory LOADS return in order among themselves whatever their cache policy, so that a counted
// vmcnt(N) which ignores stores is never too low; gfx12 has a separate store counter and would not need any of this).  The
// bit-parity backward tests pass in both builds; tests/test_isa_properties.py pins the loads-in-flight property of the default.
__device__ __forceinline__ void raw16_store(char* p, const u32x4 v, int pol) {
    PM_GLOBAL u32x4* q = as_global<u32x4>(p);
#ifdef PM_VISIBLE_STORES
    if (pol == 2) *reinterpret_cast<volatile PM_GLOBAL u32x4*>(q) = v;
    else if (pol >= 3) __hip_atomic_store(reinterpret_cast<PM_GLOBAL uint32_t*>(q), v.x, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT),
                       __hip_atomic_store(reinterpret_cast<PM_GLOBAL uint32_t*>(q) + 1, v.y, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT),
                       __hip_atomic_store(reinterpret_cast<PM_GLOBAL uint32_t*>(q) + 2, v.z, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT),
                       __hip_atomic_store(reinterpret_cast<PM_GLOBAL uint32_t*>(q) + 3, v.w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    else if (pol == 1) __builtin_nontemporal_store(v, q);
    else *q = v;
    return;
#endif
    if (pol == 2) asm volatile("global_store_dwordx4 %0, %1, off sc0 sc1\n\ts_nop 1" : : "v"(q), "v"(v) : "memory");
    else if (pol >= 3) asm volatile("global_store_dwordx4 %0, %1, off sc1\n\ts_nop 1" : : "v"(q), "v"(v) : "memory");
    else if (pol == 1) asm volatile("global_store_dwordx4 %0, %1, off nt\n\ts_nop 1" : : "v"(q), "v"(v) : "memory");
    else asm volatile("global_store_dwordx4 %0, %1, off\n\ts_nop 1" : : "v"(q), "v"(v) : "memory");
}
// ... plain stores of the kernels' own records (chunk partial sums, optimizer state)
__device__ __forceinline__ void hidden_store16(float* p, const float (&a)[4]) {
    const u32x4 v = {__float_as_uint(a[0]), __float_as_uint(a[1]), __float_as_uint(a[2]), __float_as_uint(a[3])};
#ifdef PM_VISIBLE_STORES
    *as_global<u32x4>(p) = v;
    return;
#endif
    asm volatile("global_store_dwordx4 %0, %1, off\n\ts_nop 1" : : "v"(as_global<u32x4>(p)), "v"(v) : "memory");
}
__device__ __forceinline__ void hidden_store4(float* p, float x) {
#ifdef PM_VISIBLE_STORES
    *as_global<float>(p) = x;
    return;
#endif
    asm volatile("global_store_dword %0, %1, off" : : "v"(as_global<float>(p)), "v"(x) : "memory");
}
template <int VEC>
__device__ __forceinline__ void hidden_store_vec(float* p, const float (&a)[VEC]) {
#pragma unroll
    for (int k = 0; k < VEC; k += 4) {
        const float b[4] = {a[k], a[k + 1], a[k + 2], a[k + 3]};
        hidden_store16(p + k, b);
    }
}

// counter-based random bits for stochastic rounding: one 64-bit splitmix output per (seed, row key, column pair)
__device__ __forceinline__ uint32_t sr_bits(uint64_t seed, uint64_t rowkey, int col_pair) {
    uint64_t x = seed ^ (rowkey * 0x9E3779B97F4A7C15ull) ^ (static_cast<uint64_t>(col_pair) * 0xD1B54A32D192ED03ull);
    x += 0x9E3779B97F4A7C15ull;
    x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ull;
    x = (x ^ (x >> 27)) * 0x94D049BB133111EBull;
    return static_cast<uint32_t>((x ^ (x >> 31)) >> 32);
}

struct SDstF32 {
    static constexpr int kVec = 4, kES = 4;
    __device__ static __forceinline__ void store_sr(char* p, const float (&a)[4], int nt, uint64_t, uint64_t, int) {
        store(p, a, nt);   // fp32 tables: nothing to round
    }
    // load = load_raw + widen: the main kernel's batch keeps the rows RAW until they are consumed -- arithmetic on a loaded value
    // right behind its load makes the compiler wait for the load where it stands, in the middle of the batch's load phase
    __device__ static __forceinline__ u32x4 load_raw(const char* p, int nt = 0) { return raw16_load(p, nt); }
    __device__ static __forceinline__ void widen(const u32x4 v, float (&a)[4]) { fwd::Elem<float>::widen(v, a); }
    __device__ static __forceinline__ void load(const char* p, float (&a)[4], int nt = 0) { widen(raw16_load(p, nt), a); }
    __device__ static __forceinline__ void store(char* p, const float (&a)[4], int nt = 0) {
        raw16_store(p, u32x4{__float_as_uint(a[0]), __float_as_uint(a[1]), __float_as_uint(a[2]), __float_as_uint(a[3])}, nt);
    }
};
using fwd::f32_to_bf16_rne;      // (fwd_elem.h: one definition for the library)
// fp32 -> bf16, stochastic: add 16 uniform random bits below the kept mantissa, truncate.  P(round up) equals the
// discarded fraction, so the expectation is the fp32 value; Inf/NaN pass through the nearest-even path.
__device__ __forceinline__ uint32_t f32_to_bf16_sr(float f, uint32_t r16) {
    const uint32_t u = __float_as_uint(f);
    if ((u & 0x7f800000u) == 0x7f800000u) return f32_to_bf16_rne(f);
    return (u + (r16 & 0xffffu)) >> 16;
}
struct SDstBF16 {
    static constexpr int kVec = 8, kES = 2;
    __device__ static __forceinline__ void store_sr(char* p, const float (&a)[8], int nt, uint64_t seed, uint64_t rowkey, int c) {
        uint32_t w[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const uint32_t r = sr_bits(seed, rowkey, (c >> 1) + i);
            w[i] = f32_to_bf16_sr(a[2 * i], r) | (f32_to_bf16_sr(a[2 * i + 1], r >> 16) << 16);
        }
        raw16_store(p, u32x4{w[0], w[1], w[2], w[3]}, nt);
    }
    __device__ static __forceinline__ u32x4 load_raw(const char* p, int nt = 0) { return raw16_load(p, nt); }
    __device__ static __forceinline__ void widen(const u32x4 v, float (&a)[8]) { fwd::Elem<fwd::bf16_t>::widen(v, a); }
    __device__ static __forceinline__ void load(const char* p, float (&a)[8], int nt = 0) { widen(raw16_load(p, nt), a); }
    __device__ static __forceinline__ void store(char* p, const float (&a)[8], int nt = 0) {
        uint32_t w[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) w[i] = f32_to_bf16_rne(a[2 * i]) | (f32_to_bf16_rne(a[2 * i + 1]) << 16);
        raw16_store(p, u32x4{w[0], w[1], w[2], w[3]}, nt);
    }
};
// fp32 -> fp16, stochastic.  Normal range of fp16 (|f| >= 2^-14): 13 random bits are added below the 10 kept mantissa bits and
// the low 13 bits cleared; the conversion that follows rounds to nearest, but has nothing left to round (same scheme as
// fbgemm's).  Below 2^-14 that conversion is NOT exact -- fp16 keeps fewer than 10 bits there -- and a round-to-nearest after
// the random add is no stochastic rounding at all (measured: a value 0.25 of a spacing above its lower neighbour went up in
// 0.4 % of the draws).  There the fp16 grid has the one spacing 2^-24, so the value is rounded on that grid directly:
// floor(|f| * 2^24 + u), u uniform in [0, 1) from the same 13 bits, in fixed point with 13 fraction bits (|f| * 2^37 < 2^23 is
// exact in fp32 and its truncation drops less than 2^-13 of a spacing, the resolution of the draw); 0x400 is the smallest
// normal, so a carry out of the subnormals lands on the right bits.  This is where the scheme departs from fbgemm's.
__device__ __forceinline__ uint32_t f32_to_f16_sr(float f, uint32_t r13) {
    uint32_t u = __float_as_uint(f);
    const uint32_t a = u & 0x7fffffffu;
    if (a < 0x38800000u) {
        const uint32_t q = static_cast<uint32_t>(__uint_as_float(a) * 137438953472.0f);      // |f| * 2^37, truncated
        return ((u >> 16) & 0x8000u) | ((q + (r13 & 0x1fffu)) >> 13);
    }
    if ((u & 0x7f800000u) != 0x7f800000u) u = (u + (r13 & 0x1fffu)) & 0xffffe000u;
    return static_cast<uint32_t>(__builtin_bit_cast(uint16_t, static_cast<_Float16>(__uint_as_float(u))));
}
struct SDstF16 {
    static constexpr int kVec = 8, kES = 2;
    __device__ static __forceinline__ void store_sr(char* p, const float (&a)[8], int nt, uint64_t seed, uint64_t rowkey, int c) {
        uint32_t w[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const uint32_t r = sr_bits(seed, rowkey, (c >> 1) + i);
            w[i] = f32_to_f16_sr(a[2 * i], r) | (f32_to_f16_sr(a[2 * i + 1], r >> 16) << 16);
        }
        raw16_store(p, u32x4{w[0], w[1], w[2], w[3]}, nt);
    }
    __device__ static __forceinline__ u32x4 load_raw(const char* p, int nt = 0) { return raw16_load(p, nt); }
    __device__ static __forceinline__ void widen(const u32x4 v, float (&a)[8]) { fwd::Elem<fwd::f16_t>::widen(v, a); }
    __device__ static __forceinline__ void load(const char* p, float (&a)[8], int nt = 0) { widen(raw16_load(p, nt), a); }
    __device__ static __forceinline__ void store(char* p, const float (&a)[8], int nt = 0) {
        uint32_t w[4];
#pragma unroll
        for (int i = 0; i < 4; ++i)
            w[i] = static_cast<uint32_t>(__builtin_bit_cast(uint16_t, static_cast<_Float16>(a[2 * i]))) |
                   (static_cast<uint32_t>(__builtin_bit_cast(uint16_t, static_cast<_Float16>(a[2 * i + 1]))) << 16);
        raw16_store(p, u32x4{w[0], w[1], w[2], w[3]}, nt);
    }
};

#include <cstdlib>
#include "embbag_bwd_sorted_kernels.inc"

template <typename DST, typename K, int G, int TILE>
hipError_t launch_apply_t(SortedParams sp, hipStream_t stream) {
    constexpr int NG = kBlock / G;
    constexpr int C = TILE / NG;
    int64_t grid = (sp.n + TILE - 1) / TILE;
    if (sp.xcd == 2)
        grid = static_cast<int64_t>(kXcds) * ((grid + kXcds - 1) / kXcds);
    else if (sp.seg_tiles > 0)
        grid = (sp.xcd ? static_cast<int64_t>(kXcds) * ((sp.T + kXcds - 1) / kXcds) : static_cast<int64_t>(sp.T)) * sp.seg_tiles;
    const int64_t n_chunks = (sp.n + C - 1) / C;       // every chunk below this index wrote its record
    // the fix-up takes its runs from the list the main kernel wrote: a fixed grid, one listed run per lane group and round
    static const int fix_env = [] { const char* e = getenv("PARAM_AMD_FIX_GRID"); return e ? atoi(e) : kFixGrid; }();      // once per process
    const int64_t fneed = (n_chunks + NG - 1) / NG, fgrid = fneed < fix_env ? fneed : fix_env;
    const dim3 g1(static_cast<unsigned>(grid)), g2(static_cast<unsigned>(fgrid)), blk(kBlock);
    // tile-level partial sums for runs that fill whole tiles (a Zipf head row, a 3-row table: the fix-up then adds one partial per
    // TILE instead of one per chunk).  The groups of such a tile meet at a barrier once per column pass: every lane must make the
    // same number of passes (row-wise Adagrad: one pass, all lanes).
    static const int join_env = [] { const char* e = getenv("PARAM_AMD_JOIN_TILES"); return e ? atoi(e) : 1; }();        // once per process
    const bool adagrad = sp.mom || sp.state;       // row-wise / element-wise: one column pass either way
    sp.join_tiles = (join_env != 0 && sp.exact_run < TILE && !(adagrad && sp.psw) && (adagrad || sp.max_dim % (G * DST::kVec) == 0)) ? 1 : 0;
    // one (main, fix-up) pair per bag phase, in stream order: phase 0 has updated a row before phase 1 touches it
    for (int ph = 0; ph < sp.H; ++ph) {
        sp.phase = ph;
        // Adagrad: one column pass with all G lanes (row-wise: cross-lane reduction; element-wise keeps the rule)
        if (adagrad && (sp.max_dim > G * DST::kVec || sp.H != 1 || (sp.mom && sp.state))) return hipErrorInvalidValue;
        dispatch_opt(sp.state != nullptr, sp.mom != nullptr, [&](auto opt) {
            dispatch_bool(sp.psw != nullptr, [&](auto w) {
                constexpr int OPT = decltype(opt)::value;
                constexpr bool W = decltype(w)::value;
                hipLaunchKernelGGL((bwd_sorted_main_kernel<DST, K, G, W, OPT, TILE>), g1, blk, static_cast<size_t>(sp.T) * (OPT != 0 ? 28 : 20),
                                   stream, sp);
                hipLaunchKernelGGL((bwd_sorted_fixup_kernel<DST, K, G, W, OPT, TILE>), g2, blk, 0, stream, sp, n_chunks);
            });
        });
    }
    return hipGetLastError();
}

template <typename DST, typename K, int G>
hipError_t launch_apply_w(const SortedParams& sp, hipStream_t stream) {
    switch (sp.tile) {
        case 256: return launch_apply_t<DST, K, G, 256>(sp, stream);
        case 512: return launch_apply_t<DST, K, G, 512>(sp, stream);
        default: return launch_apply_t<DST, K, G, kSortTile>(sp, stream);
    }
}

template <typename DST, typename K>
hipError_t launch_apply_g(const SortedParams& sp, int max_dim, hipStream_t stream) {
    return dispatch_group_lanes(group_lanes(max_dim, DST::kVec),
                                [&](auto g) { return launch_apply_w<DST, K, decltype(g)::value>(sp, stream); });
}


// the hybrid backward's bag-major apply (bwd_unique_kernel): same request geometry as the forward
template <typename DST>
hipError_t launch_unique_g(const SortedParams& sp, const KParams& kp, const UniqueArgs& ua, int max_dim, hipStream_t stream) {
    unsigned n_wg = static_cast<unsigned>(kp.T) * static_cast<unsigned>(kp.tiles_per_table);
    if (sp.unique_wgs_per_cu > 0 && n_wg > 256u * static_cast<unsigned>(sp.unique_wgs_per_cu)) n_wg = 256u * static_cast<unsigned>(sp.unique_wgs_per_cu);
    const dim3 grid(n_wg), blk(kBlock);
    const size_t lds = tile_lds_bytes(kp.bags_per_block, kp.idx_cap, false);
    const int g = group_lanes(max_dim, DST::kVec);
    if ((sp.mom || sp.state) && max_dim > g * DST::kVec) return hipErrorInvalidValue;
    dispatch_group_lanes(g, [&](auto gl) {
        dispatch_opt(sp.state != nullptr, sp.mom != nullptr, [&](auto opt) {
            hipLaunchKernelGGL((bwd_unique_kernel<DST, decltype(gl)::value, decltype(opt)::value>), grid, blk, lds, stream, sp, kp, ua.hyb_tab,
                               ua.bloom, ua.emit_keys, ua.emit_vals, ua.key_bytes, ua.tile_cnt, ua.tile_cnt_stride, ua.bloom_wbits);
        });
    });
    return hipGetLastError();
}


// the hybrid backward's left-overs (hyb_rest_kernel): T_h x parts workgroups of 1024 threads, 81 KB of dynamic LDS
template <typename DST>
hipError_t launch_rest_g(const SortedParams& sp, const KParams& kp, const RestArgs& ra, int max_dim, hipStream_t stream) {
    if (ra.T_h < 1 || ra.parts < 1) return hipErrorInvalidValue;
    const dim3 grid(static_cast<unsigned>(ra.T_h) * static_cast<unsigned>(ra.parts)), blk(kRestThreads);
    const size_t lds = static_cast<size_t>(2 * kRestCap + kRestAux) * sizeof(uint32_t);
    const int g = group_lanes(max_dim, DST::kVec);
    if ((sp.mom || sp.state) && max_dim > g * DST::kVec) return hipErrorInvalidValue;
    return dispatch_group_lanes(g, [&](auto gl) {
        return dispatch_opt(sp.state != nullptr, sp.mom != nullptr, [&](auto opt) {
            constexpr auto kernel = hyb_rest_kernel<DST, decltype(gl)::value, decltype(opt)::value>;
            // (the attribute is asked for once per instantiation and process: this lambda's body is one function per (G, OPT))
            static const hipError_t attr = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                                               static_cast<int>(lds));
            if (attr != hipSuccess) return attr;
            hipLaunchKernelGGL(kernel, grid, blk, lds, stream, sp, kp, ra);
            return hipGetLastError();
        });
    });
}
