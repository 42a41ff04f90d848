// Micro-benchmark: random-gather ceilings of one MI355X for the access shapes
// of the miBF probe (calibration for the roofline discussion in DESIGN.md).
//   mode 0: independent random 16-B loads          (one sector per load)
//   mode 1: independent random 4-B loads
//   mode 2: two DEPENDENT random loads per item: 16 B from table A (small),
//           then 4/8 B from table B (large) at an index derived from the first
//   mode 3: like 2 but UNR items in flight per lane
//   modes 4-10: bucket-shaped accesses (10 = what k_query does: a quad reads one 64-B line)
// Round 4 (locality / cache-residency questions, DESIGN 4 "the ceiling of the steady state"):
//   mode 11: quad 64-B lines drawn PAGE-BINNED in address order: the grid sweeps table A once,
//            item n (grid order) falls at a random line of region n / L, regions of R bytes
//            (env GB_REGION bytes, GB_DENSITY lines drawn per line of the region, default 0.6)
//   mode 17: quad 64-B lines, the 16 lines of one wave step inside ONE random region of R bytes
//   mode 18: like 17 for the 64 lines of a workgroup step
//   mode 12: random atomicOr (u32) on table B        mode 13: random atomicCAS (u64) on table B
//   mode 14: random 1-byte stores on table B         mode 15: 8 lanes read a 128-B bucket
//   mode 16: quad reads a 64-B line of A, one lane writes 4 B of it back (a dirty random line)
//   mode 20: mode 10's random lines in the loop shape of modes 11 / 17 / 18 (their reference)
//   mode 19: random u32 load from table B, one per lane, keyed like a Bloom look-up (same as 1, kept for the tables)
// Round 5 (where a rank's insert count should live, DESIGN 5c "collect"): one item = one record of k_batch_collect
//   mode 21: TODAY: 16-B header of a random 64-B bucket of A, then (dependent) CAS u64 on a random word of B
//            (the rank's count | claim), then 4 B of the bucket written back (the ID)
//   mode 22: UNIT: A as 128-B units {bucket line, count line}: header of line 0 and claim word of line 1 loaded
//            together, CAS u64 on the claim word, returning atomicAdd u32 on a count of line 1, 4 B of line 0 written
//   mode 23: like 22 without the atomicAdd (claim and count in one CAS word of line 1)
//   mode 27: like 23 plus a plain load and a plain store of a u32 count in line 1 (the claim is per BUCKET, its winner
//            owns the slot: the count needs no atomic)
//   mode 30: like 23 with the count line GB_L1OFF bytes (a power of two >= 64) behind its bucket line: A in blocks of
//            2 x GB_L1OFF bytes, first half bucket lines, second half their count lines (is the unit's gain the shared
//            DRAM page or the shared address translation?)
//   mode 31: mode 10's quad read of the bucket lines of that blocked layout
//   mode 32: like 23, but the count word's address DEPENDS on the header (its slot = the set bit's index): header,
//            then atomic load of the word, then CAS — the shape of k_batch_collect
//   mode 33: like 32 with a plain load of line 1 issued together with the header (a prefetch), the word itself read
//            with a plain load behind the header
//   mode 34: like 33, the ID slot read back behind the CAS (as the owner's touch does) and three 8-byte record words
//            written per item at a fixed index (coalesced)
//   mode 35: 33 + the read-back only; mode 36: 33 + the record words only; mode 37: 34 with the ID slot read IN FRONT of the CAS
//   mode 50: the record shape by its parts (env GB_SHAPE, a bit mask): header of line 0, count word of line 1 (slot from the
//            header), CAS, the ID slot of line 0 read and written, three record words.  bit 0: no load in front of the CAS
//            (it succeeds at once); bit 1: the ID by atomicExch instead of load + store; bit 2: the ID loaded in front of
//            the CAS (with the count word); bit 3: the ID stored write-through (agent scope); bit 4: no record words;
//            bit 5: the header through two agent-scope 8-byte loads; bit 6: ID store skipped (a touch that does not write)
//   mode 24: mode 10's quad read of a 64-B line where the lines lie 128 B apart (the query on the unit layout)
//   mode 25: one 128-B unit read whole by 8 lanes, one lane writes 4 B into each half
//   mode 28: mode 24 with the quad's pieces rotated per round (lane L loads piece (L - g) & 3 of quad lane g's line): the
//            load order of quad_decode, where a probe's header arrives in the lane that owns the probe
//   mode 26: like 21 with the count word in a SEPARATE line of a bucket-indexed table B (64 B per bucket, same index)
// usage: gather_bench <tableA_MiB> <tableB_MiB> <items_per_lane> <mode> [unroll] [workgroups]
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdlib>
#include <cstdint>

#define CK(x) do { hipError_t e = (x); if (e != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e)); exit(1);} } while (0)

__device__ inline uint64_t mix64(uint64_t x) { x += 0x9E3779B97F4A7C15ULL; x = (x ^ (x >> 30)) * 0xBF58476D1CE4E5B9ULL; x = (x ^ (x >> 27)) * 0x94D049BB133111EBULL; return x ^ (x >> 31); }

template<int UNR>
__global__ void __launch_bounds__(256) k_gather(const uint4* __restrict__ A, uint64_t nA, const uint2* __restrict__ B, uint64_t nB, int items, int mode, uint64_t* __restrict__ out, uint64_t region_lines, uint64_t lines_per_region)
{
  const uint64_t gid = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  uint64_t acc = 0;
  for (int it = 0; it < items; it += UNR) {
    uint64_t ia[UNR];
    uint4 va[UNR];
#pragma unroll
    for (int u = 0; u < UNR; ++u) {
      ia[u] = mix64(gid * 1315423911ULL + (uint64_t)(it + u) * 0x9E3779B97F4A7C15ULL);
    }
    if (mode == 0) {
#pragma unroll
      for (int u = 0; u < UNR; ++u) va[u] = A[ia[u] % nA];
#pragma unroll
      for (int u = 0; u < UNR; ++u) acc += va[u].x + va[u].w;
    } else if (mode == 1) {
      uint32_t v[UNR];
#pragma unroll
      for (int u = 0; u < UNR; ++u) v[u] = reinterpret_cast<const uint32_t*>(B)[ia[u] % (nB * 2)];
#pragma unroll
      for (int u = 0; u < UNR; ++u) acc += v[u];
    } else if (mode == 8) { // 8-B header, then a DEPENDENT 4-B slot of the same 64-B bucket
      const uint64_t nb = nA / 4;
      uint2 h2[UNR];
      uint32_t v[UNR];
#pragma unroll
      for (int u = 0; u < UNR; ++u) h2[u] = reinterpret_cast<const uint2*>(A)[(ia[u] % nb) * 8];
#pragma unroll
      for (int u = 0; u < UNR; ++u) v[u] = reinterpret_cast<const uint32_t*>(A)[(ia[u] % nb) * 16 + 2 + ((h2[u].y ^ ia[u]) % 14)];
#pragma unroll
      for (int u = 0; u < UNR; ++u) acc += h2[u].x + v[u];
    } else if (mode == 20) { // mode 10's access (a quad reads one random 64-B line) in the loop shape of modes 11 / 17 / 18
      const uint64_t nbmask = nA / 4 - 1;
      const int lane = threadIdx.x & 63;
      const int sub = lane & 3;
#pragma unroll
      for (int u = 0; u < UNR; ++u) {
        const uint64_t idx = mix64((gid / 4) * 77ULL + (uint64_t)(it + u) * 0xD1B54A32D192ED03ULL) & nbmask;
        const uint4 t = A[idx * 4 + sub];
        const uint32_t got = __shfl(t.w, (lane & ~3) + (int)(idx & 3), 64);
        acc += got + t.x;
      }
    } else if (mode == 9 || mode == 10) {
      // cooperative: G lanes read one whole 64-B bucket with one coalesced access;
      // every lane still owns `items` probes, processed G at a time via shuffles
      const int G = (mode == 9) ? 8 : 4;
      const uint64_t nb = nA / 4;
      const int lane = threadIdx.x & 63;
      const int sub = lane % G;
#pragma unroll
      for (int u = 0; u < UNR; ++u) {
        for (int g = 0; g < G; ++g) {
          // the probe of lane (group base + g)
          const uint64_t idx = __shfl(ia[u], (lane / G) * G + g, 64) % nb;
          if (mode == 9) {
            uint2 t = reinterpret_cast<const uint2*>(A)[idx * 8 + sub];
            const uint32_t want = (uint32_t)(idx >> 3) % 8u;
            uint32_t got = __shfl(t.y, (lane / G) * G + want, 64);
            if (sub == g) acc += got + t.x;
          } else {
            uint4 t = A[idx * 4 + sub];
            const uint32_t want = (uint32_t)(idx >> 3) % 4u;
            uint32_t got = __shfl(t.w, (lane / G) * G + want, 64);
            if (sub == g) acc += got + t.x;
          }
        }
      }
    } else if (mode == 11 || mode == 17 || mode == 18) {
      // (table and region sizes are powers of two: masks and one reciprocal multiply, no 64-bit division —
      // a first form spent its time in three `%` per item and measured the ALU, not the memory system)
      const uint64_t nb = nA / 4; // 64-B lines of table A
      const int lane = threadIdx.x & 63;
      const int sub = lane & 3;
      const uint32_t nquads = gridDim.x * blockDim.x / 4;
      const uint32_t inv = (uint32_t)(0x100000000ull / lines_per_region); // region of item n ~ (n * inv) >> 32
      const uint64_t rmask = region_lines - 1, nbmask = nb - 1, nregmask = nb / region_lines - 1;
#pragma unroll
      for (int u = 0; u < UNR; ++u) {
        uint64_t idx;
        if (mode == 11) {
          const uint32_t n = (uint32_t)(it + u) * nquads + (uint32_t)(gid / 4); // grid order: the sweep
          const uint64_t region = ((uint64_t)n * inv) >> 32;
          idx = (region * region_lines + (mix64(n) & rmask)) & nbmask;
        } else {
          // the lines of one wave (17) / workgroup (18) step share a random region
          const uint64_t scope = (mode == 17) ? gid / 64 : gid / 256;
          const uint64_t region = mix64(scope * 0x9E3779B97F4A7C15ULL + (uint64_t)(it + u)) & nregmask;
          idx = region * region_lines + (mix64((gid / 4) * 77ULL + (uint64_t)(it + u) * 0xD1B54A32D192ED03ULL) & rmask);
        }
        const uint4 t = A[idx * 4 + sub];
        const uint32_t got = __shfl(t.w, (lane & ~3) + (int)(idx & 3), 64);
        acc += got + t.x;
      }
    } else if (mode == 12) {
      uint32_t* T = const_cast<uint32_t*>(reinterpret_cast<const uint32_t*>(B));
#pragma unroll
      for (int u = 0; u < UNR; ++u) atomicOr(&T[ia[u] % (nB * 2)], 1u << (ia[u] >> 59));
    } else if (mode == 13) {
      unsigned long long* T = const_cast<unsigned long long*>(reinterpret_cast<const unsigned long long*>(B));
      unsigned long long v[UNR];
#pragma unroll
      for (int u = 0; u < UNR; ++u) v[u] = atomicCAS(&T[ia[u] % nB], 0x0202020202020202ULL, ia[u] | 1ull);
#pragma unroll
      for (int u = 0; u < UNR; ++u) acc += v[u];
    } else if (mode == 14) {
      uint8_t* T = const_cast<uint8_t*>(reinterpret_cast<const uint8_t*>(B));
#pragma unroll
      for (int u = 0; u < UNR; ++u) T[ia[u] % (nB * 8)] = 1;
    } else if (mode == 15) {
      const uint64_t nb = nA / 8; // 128-B buckets
      const int lane = threadIdx.x & 63;
      const int sub = lane & 7;
#pragma unroll
      for (int u = 0; u < UNR; ++u) {
        for (int g = 0; g < 8; ++g) {
          const uint64_t idx = __shfl(ia[u], (lane & ~7) + g, 64) % nb;
          const uint4 t = A[idx * 8 + sub];
          const uint32_t got = __shfl(t.w, (lane & ~7) + (int)(idx & 7), 64);
          if (sub == g) acc += got + t.x;
        }
      }
    } else if (mode == 16) {
      const uint64_t nb = nA / 4;
      const int lane = threadIdx.x & 63;
      const int sub = lane & 3;
      uint4* W = const_cast<uint4*>(A);
#pragma unroll
      for (int u = 0; u < UNR; ++u) {
        for (int g = 0; g < 4; ++g) {
          const uint64_t idx = __shfl(ia[u], (lane & ~3) + g, 64) % nb;
          const uint4 t = A[idx * 4 + sub];
          if (sub == g) {
            acc += t.x;
            reinterpret_cast<uint32_t*>(W)[idx * 16 + 3 + (ia[u] >> 50) % 13] = (uint32_t)ia[u] | 1u;
          }
        }
      }
    } else if (mode == 21 || mode == 26) {
      const uint64_t nb = nA / 4;
      uint32_t* W = const_cast<uint32_t*>(reinterpret_cast<const uint32_t*>(A));
      unsigned long long* T = const_cast<unsigned long long*>(reinterpret_cast<const unsigned long long*>(B));
      unsigned long long v[UNR];
#pragma unroll
      for (int u = 0; u < UNR; ++u) va[u] = A[(ia[u] % nb) * 4];
#pragma unroll
      for (int u = 0; u < UNR; ++u) {
        const uint32_t lr = (uint32_t)((va[u].y ^ ia[u]) % 13);
        const uint64_t ib = (mode == 21) ? (mix64(ia[u] ^ va[u].x) % nB) : (((ia[u] % nb) * 8 + (lr & 7u)) % nB);
        v[u] = atomicCAS(&T[ib], 0x0202020202020202ULL, 0x0202020202020202ULL + (va[u].z & 1u));
      }
#pragma unroll
      for (int u = 0; u < UNR; ++u) {
        const uint32_t lr = (uint32_t)((va[u].y ^ ia[u]) % 13);
        W[(ia[u] % nb) * 16 + 3 + lr] = (uint32_t)v[u] | 1u;
        acc += v[u];
      }
    } else if (mode == 22 || mode == 23 || mode == 27) {
      const uint64_t nu = nA / 8; // 128-B units
      uint32_t* W = const_cast<uint32_t*>(reinterpret_cast<const uint32_t*>(A));
      unsigned long long* T = const_cast<unsigned long long*>(reinterpret_cast<const unsigned long long*>(A));
      unsigned long long cw[UNR], v[UNR];
      uint32_t c[UNR];
#pragma unroll
      for (int u = 0; u < UNR; ++u) {
        va[u] = A[(ia[u] % nu) * 8];
        cw[u] = __hip_atomic_load(&T[(ia[u] % nu) * 16 + 15], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
#pragma unroll
      for (int u = 0; u < UNR; ++u) v[u] = atomicCAS(&T[(ia[u] % nu) * 16 + 15], cw[u], cw[u] + (va[u].z & 1u));
#pragma unroll
      for (int u = 0; u < UNR; ++u) {
        const uint32_t lr = (uint32_t)((va[u].y ^ ia[u]) % 13);
        c[u] = (mode == 22) ? atomicAdd(&W[(ia[u] % nu) * 32 + 16 + lr], 1u) : (mode == 27) ? W[(ia[u] % nu) * 32 + 16 + lr] : 0u;
      }
      if (mode == 27) {
#pragma unroll
        for (int u = 0; u < UNR; ++u) {
          const uint32_t lr = (uint32_t)((va[u].y ^ ia[u]) % 13);
          W[(ia[u] % nu) * 32 + 16 + lr] = c[u] + 1u;
        }
      }
#pragma unroll
      for (int u = 0; u < UNR; ++u) {
        const uint32_t lr = (uint32_t)((va[u].y ^ ia[u]) % 13);
        W[(ia[u] % nu) * 32 + 3 + lr] = (uint32_t)v[u] | c[u] | 1u;
        acc += v[u];
      }
    } else if (mode >= 32 && mode <= 37) {
      const uint64_t nu = nA / 8; // 128-B units
      uint32_t* W = const_cast<uint32_t*>(reinterpret_cast<const uint32_t*>(A));
      unsigned long long* T = const_cast<unsigned long long*>(reinterpret_cast<const unsigned long long*>(A));
      unsigned long long* R = const_cast<unsigned long long*>(reinterpret_cast<const unsigned long long*>(B));
      unsigned long long cw[UNR], v[UNR], pf[UNR];
      uint32_t idv[UNR];
#pragma unroll
      for (int u = 0; u < UNR; ++u) {
        va[u] = A[(ia[u] % nu) * 8];
        pf[u] = (mode >= 33) ? T[(ia[u] % nu) * 16 + 8] : 0ull;
      }
#pragma unroll
      for (int u = 0; u < UNR; ++u) {
        const uint32_t lr = (uint32_t)((va[u].y ^ ia[u]) % 8);
        unsigned long long* q = &T[(ia[u] % nu) * 16 + 8 + lr];
        cw[u] = (mode >= 33) ? *q : __hip_atomic_load(q, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
#pragma unroll
      for (int u = 0; u < UNR; ++u) {
        const uint32_t lr = (uint32_t)((va[u].y ^ ia[u]) % 8);
        v[u] = atomicCAS(&T[(ia[u] % nu) * 16 + 8 + lr], cw[u], cw[u] + (va[u].z & 1u) + (pf[u] & 0u));
      }
#pragma unroll
      for (int u = 0; u < UNR; ++u) {
        const uint32_t lr = (uint32_t)((va[u].y ^ ia[u]) % 8);
        // 34 / 35: the ID slot read back behind the CAS; 37: read in front of it (with the count word)
        idv[u] = (mode == 34 || mode == 35) ? W[(ia[u] % nu) * 32 + 3 + lr + (uint32_t)(v[u] & 0ull)] : (mode == 37) ? W[(ia[u] % nu) * 32 + 3 + lr + (uint32_t)(cw[u] & 0ull)] : 0u;
      }
#pragma unroll
      for (int u = 0; u < UNR; ++u) {
        const uint32_t lr = (uint32_t)((va[u].y ^ ia[u]) % 8);
        W[(ia[u] % nu) * 32 + 3 + lr] = (uint32_t)v[u] | idv[u] | 1u;
        if (mode == 34 || mode == 36 || mode == 37) {
          const uint64_t ridx = ((uint64_t)(it + u) * gridDim.x * blockDim.x + gid) % (nB / 3);
          R[ridx] = v[u];
          R[nB / 3 + ridx] = cw[u];
          R[2 * (nB / 3) + ridx] = idv[u];
        }
        acc += v[u];
      }
    } else if (mode == 50) {
      const uint32_t shape = (uint32_t)lines_per_region; // GB_SHAPE rides here
      const uint64_t nu = nA / 8;
      uint32_t* W = const_cast<uint32_t*>(reinterpret_cast<const uint32_t*>(A));
      unsigned long long* T = const_cast<unsigned long long*>(reinterpret_cast<const unsigned long long*>(A));
      unsigned long long* R = const_cast<unsigned long long*>(reinterpret_cast<const unsigned long long*>(B));
      unsigned long long cw[UNR], v[UNR];
      uint32_t idv[UNR];
#pragma unroll
      for (int u = 0; u < UNR; ++u) {
        if (shape & 32u) {
          const unsigned long long a = __hip_atomic_load(&T[(ia[u] % nu) * 16], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          const unsigned long long b = __hip_atomic_load(&T[(ia[u] % nu) * 16 + 1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          va[u] = make_uint4((uint32_t)a, (uint32_t)(a >> 32), (uint32_t)b, (uint32_t)(b >> 32));
        } else {
          va[u] = A[(ia[u] % nu) * 8];
        }
      }
#pragma unroll
      for (int u = 0; u < UNR; ++u) {
        const uint32_t lr = (uint32_t)((va[u].y ^ ia[u]) % 8);
        cw[u] = (shape & 1u) ? 0x0101010101010101ULL : __hip_atomic_load(&T[(ia[u] % nu) * 16 + 8 + lr], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        idv[u] = (shape & 4u) ? W[(ia[u] % nu) * 32 + 3 + lr] : 0u;
      }
#pragma unroll
      for (int u = 0; u < UNR; ++u) {
        const uint32_t lr = (uint32_t)((va[u].y ^ ia[u]) % 8);
        v[u] = atomicCAS(&T[(ia[u] % nu) * 16 + 8 + lr], cw[u], cw[u] + (va[u].z & 0u));
      }
#pragma unroll
      for (int u = 0; u < UNR; ++u) {
        const uint32_t lr = (uint32_t)((va[u].y ^ ia[u]) % 8);
        uint32_t* p = &W[(ia[u] % nu) * 32 + 3 + lr + (uint32_t)(v[u] & 0ull)];
        if (shape & 2u) {
          idv[u] = atomicExch(p, (uint32_t)v[u] | 1u);
        } else {
          if (!(shape & 4u)) idv[u] = *p;
        }
      }
#pragma unroll
      for (int u = 0; u < UNR; ++u) {
        const uint32_t lr = (uint32_t)((va[u].y ^ ia[u]) % 8);
        uint32_t* p = &W[(ia[u] % nu) * 32 + 3 + lr];
        if (!(shape & 2u) && !(shape & 64u)) {
          if (shape & 8u) __hip_atomic_store(p, idv[u] | 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          else *p = idv[u] | 1u;
        }
        if (!(shape & 16u)) {
          const uint64_t ridx = ((uint64_t)(it + u) * gridDim.x * blockDim.x + gid) % (nB / 3);
          R[ridx] = v[u];
          R[nB / 3 + ridx] = cw[u];
          R[2 * (nB / 3) + ridx] = idv[u];
        }
        acc += v[u] + idv[u];
      }
    } else if (mode == 30) {
      // region_lines carries GB_L1OFF / 64 here
      const uint64_t nl = nA / 8; // bucket lines (half the table)
      const uint64_t per = region_lines; // lines per half block
      uint32_t* W = const_cast<uint32_t*>(reinterpret_cast<const uint32_t*>(A));
      unsigned long long* T = const_cast<unsigned long long*>(reinterpret_cast<const unsigned long long*>(A));
      unsigned long long cw[UNR], v[UNR];
      uint64_t l0[UNR], l1[UNR];
#pragma unroll
      for (int u = 0; u < UNR; ++u) {
        const uint64_t b = ia[u] % nl;
        l0[u] = (b / per) * 2 * per + (b % per); // 64-B line index of the bucket line
        l1[u] = l0[u] + per;
        va[u] = A[l0[u] * 4];
        cw[u] = __hip_atomic_load(&T[l1[u] * 8 + 7], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
#pragma unroll
      for (int u = 0; u < UNR; ++u) v[u] = atomicCAS(&T[l1[u] * 8 + 7], cw[u], cw[u] + (va[u].z & 1u));
#pragma unroll
      for (int u = 0; u < UNR; ++u) {
        const uint32_t lr = (uint32_t)((va[u].y ^ ia[u]) % 13);
        W[l0[u] * 16 + 3 + lr] = (uint32_t)v[u] | 1u;
        acc += v[u];
      }
    } else if (mode == 31) {
      const uint64_t nl = nA / 8;
      const uint64_t per = region_lines;
      const int lane = threadIdx.x & 63;
      const int sub = lane & 3;
#pragma unroll
      for (int u = 0; u < UNR; ++u) {
        for (int g = 0; g < 4; ++g) {
          const uint64_t b = __shfl(ia[u], (lane / 4) * 4 + g, 64) % nl;
          const uint64_t idx = (b / per) * 2 * per + (b % per);
          uint4 t = A[idx * 4 + sub];
          const uint32_t want = (uint32_t)(idx >> 3) % 4u;
          uint32_t got = __shfl(t.w, (lane / 4) * 4 + want, 64);
          if (sub == g) acc += got + t.x;
        }
      }
    } else if (mode == 24) {
      const uint64_t nu = nA / 8;
      const int lane = threadIdx.x & 63;
      const int sub = lane & 3;
#pragma unroll
      for (int u = 0; u < UNR; ++u) {
        for (int g = 0; g < 4; ++g) {
          const uint64_t idx = __shfl(ia[u], (lane / 4) * 4 + g, 64) % nu;
          uint4 t = A[idx * 8 + sub];
          const uint32_t want = (uint32_t)(idx >> 3) % 4u;
          uint32_t got = __shfl(t.w, (lane / 4) * 4 + want, 64);
          if (sub == g) acc += got + t.x;
        }
      }
    } else if (mode == 28) { // mode 24 with the pieces ROTATED: in round g lane L loads piece (L - g) & 3, so lane g gets its own line's header
      const uint64_t nu = nA / 8;
      const int lane = threadIdx.x & 63;
      const int sub = lane & 3;
#pragma unroll
      for (int u = 0; u < UNR; ++u) {
        for (int g = 0; g < 4; ++g) {
          const uint64_t idx = __shfl(ia[u], (lane / 4) * 4 + g, 64) % nu;
          uint4 t = A[idx * 8 + ((sub - g) & 3)];
          const uint32_t want = (uint32_t)(idx >> 3) % 4u; // the piece that holds the word asked for: in quad lane (g + want) & 3
          uint32_t got = __shfl(t.w, (lane / 4) * 4 + (int)((g + want) & 3u), 64);
          if (sub == g) acc += got + t.x;
        }
      }
    } else if (mode == 25) {
      const uint64_t nu = nA / 8;
      const int lane = threadIdx.x & 63;
      const int sub = lane & 7;
      uint32_t* W = const_cast<uint32_t*>(reinterpret_cast<const uint32_t*>(A));
#pragma unroll
      for (int u = 0; u < UNR; ++u) {
        for (int g = 0; g < 8; ++g) {
          const uint64_t idx = __shfl(ia[u], (lane & ~7) + g, 64) % nu;
          const uint4 t = A[idx * 8 + sub];
          if (sub == g) {
            acc += t.x;
            W[idx * 32 + 3 + (ia[u] >> 50) % 13] = (uint32_t)ia[u] | 1u;
            W[idx * 32 + 16 + (ia[u] >> 50) % 13] = (uint32_t)ia[u] | 1u;
          }
        }
      }
    } else if (mode == 19) {
      uint32_t v[UNR];
#pragma unroll
      for (int u = 0; u < UNR; ++u) v[u] = reinterpret_cast<const uint32_t*>(B)[(ia[u] >> 5) % (nB * 2)];
#pragma unroll
      for (int u = 0; u < UNR; ++u) acc += (v[u] >> (ia[u] & 31)) & 1u;
    } else if (mode == 4 || mode == 5 || mode == 6 || mode == 7) {
      // bucket-shaped accesses on table A viewed as 64-byte buckets
      const uint64_t nb = nA / 4;
      uint32_t v[UNR];
      if (mode == 4) { // 16-B header, then a DEPENDENT 4-B slot of the same 64-B bucket
#pragma unroll
        for (int u = 0; u < UNR; ++u) va[u] = A[(ia[u] % nb) * 4];
#pragma unroll
        for (int u = 0; u < UNR; ++u) v[u] = reinterpret_cast<const uint32_t*>(A)[(ia[u] % nb) * 16 + 3 + ((va[u].y ^ ia[u]) % 13)];
      } else if (mode == 5) { // header and slot issued together (independent)
#pragma unroll
        for (int u = 0; u < UNR; ++u) va[u] = A[(ia[u] % nb) * 4];
#pragma unroll
        for (int u = 0; u < UNR; ++u) v[u] = reinterpret_cast<const uint32_t*>(A)[(ia[u] % nb) * 16 + 3 + (ia[u] >> 40) % 13];
      } else if (mode == 6) { // one 8-B load per bucket
#pragma unroll
        for (int u = 0; u < UNR; ++u) { uint2 t = reinterpret_cast<const uint2*>(A)[(ia[u] % nb) * 8]; va[u] = make_uint4(t.x, t.y, 0, 0); v[u] = 0; }
      } else { // one 16-B load per bucket
#pragma unroll
        for (int u = 0; u < UNR; ++u) { va[u] = A[(ia[u] % nb) * 4]; v[u] = 0; }
      }
#pragma unroll
      for (int u = 0; u < UNR; ++u) acc += va[u].x + va[u].w + v[u];
    } else {
#pragma unroll
      for (int u = 0; u < UNR; ++u) va[u] = A[ia[u] % nA];
      uint32_t v[UNR];
#pragma unroll
      for (int u = 0; u < UNR; ++u) {
        uint64_t ib = (ia[u] ^ ((uint64_t)va[u].x << 7) ^ va[u].y) % nB; // depends on the first load
        v[u] = B[ib].x;
      }
#pragma unroll
      for (int u = 0; u < UNR; ++u) acc += v[u];
    }
  }
  if (acc == 0x123456789ULL) out[0] = acc;
}

int main(int argc, char** argv)
{
  uint64_t aMiB = argc > 1 ? atoll(argv[1]) : 512, bMiB = argc > 2 ? atoll(argv[2]) : 20480;
  int items = argc > 3 ? atoi(argv[3]) : 64, mode = argc > 4 ? atoi(argv[4]) : 2, unr = argc > 5 ? atoi(argv[5]) : 4;
  int wgs = argc > 6 ? atoi(argv[6]) : 256 * 8 * 4;
  uint64_t nA = aMiB * (1ull << 20) / 16, nB = bMiB * (1ull << 20) / 8;
  uint4* A; uint2* B; uint64_t* out;
  CK(hipMalloc(&A, nA * 16)); CK(hipMalloc(&B, nB * 8)); CK(hipMalloc(&out, 8));
  CK(hipMemset(A, 1, nA * 16)); CK(hipMemset(B, 2, nB * 8));
  const uint64_t region_bytes = getenv("GB_REGION") ? strtoull(getenv("GB_REGION"), nullptr, 10) : 2048;
  const double density = getenv("GB_DENSITY") ? atof(getenv("GB_DENSITY")) : 0.6;
  uint64_t region_lines = region_bytes / 64 ? region_bytes / 64 : 1;
  if (mode == 30 || mode == 31) region_lines = (getenv("GB_L1OFF") ? strtoull(getenv("GB_L1OFF"), nullptr, 10) : 64) / 64;
  uint64_t lines_per_region = (uint64_t)(region_lines * density + 0.5);
  if (lines_per_region == 0) lines_per_region = 1;
  if (mode == 50) lines_per_region = getenv("GB_SHAPE") ? strtoull(getenv("GB_SHAPE"), nullptr, 10) : 0;
  if (mode == 11) { // one sweep of the table: items per lane from the table size
    const uint64_t nquads = (uint64_t)wgs * 256 / 4;
    const uint64_t total = (nA / 4) / region_lines * lines_per_region;
    items = (int)(total / nquads / unr * unr);
    if (items < unr) items = unr;
  }
  hipEvent_t e0, e1; CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1));
  for (int rep = 0; rep < 3; ++rep) {
    CK(hipEventRecord(e0));
    if (unr == 1) k_gather<1><<<wgs, 256>>>(A, nA, B, nB, items, mode, out, region_lines, lines_per_region);
    else if (unr == 2) k_gather<2><<<wgs, 256>>>(A, nA, B, nB, items, mode, out, region_lines, lines_per_region);
    else if (unr == 4) k_gather<4><<<wgs, 256>>>(A, nA, B, nB, items, mode, out, region_lines, lines_per_region);
    else if (unr == 8) k_gather<8><<<wgs, 256>>>(A, nA, B, nB, items, mode, out, region_lines, lines_per_region);
    else k_gather<16><<<wgs, 256>>>(A, nA, B, nB, items, mode, out, region_lines, lines_per_region);
    CK(hipEventRecord(e1)); CK(hipEventSynchronize(e1));
    float ms; CK(hipEventElapsedTime(&ms, e0, e1));
    double n = (double)wgs * 256 * items;
    if (mode == 11 || mode == 17 || mode == 18 || mode == 20) n /= 4; // one line per QUAD and item here
    if (rep == 2 && (mode == 11 || mode == 17 || mode == 18)) printf("region=%lluB density=%.2f items=%d ", (unsigned long long)region_bytes, density, items);
    if (rep == 2) printf("mode %d A=%lluMiB B=%lluMiB unr=%d wgs=%d: %.2f ms, %.2f G items/s, %.2f G sector-loads/s -> %.2f TB/s at 64 B/sector\n", mode, (unsigned long long)aMiB, (unsigned long long)bMiB, unr, wgs, ms, n / ms / 1e6, n * ((mode == 2 || mode == 3) ? 2 : 1) / ms / 1e6, n * ((mode == 2 || mode == 3) ? 2 : 1) * 64 / ms / 1e9);
  }
  return 0;
}
