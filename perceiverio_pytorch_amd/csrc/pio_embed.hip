// Front end of the language model in one pass (pio_embed_tokens): the token embedding gathered by id plus the learned
// position embedding (io_processors.py EmbeddingPreprocessor: embed(ids) + pos_embs, preprocessors.py:18-54), written once
// into the encoder's input.  Per sample b, token t, channel c, with id = ids[b ids_sb + t]:
//
//   0 <= id < V:   y[b, t, c] = fadd_rn(table[id, c], pos[t, c])      tokens[b, t, c] = table[id, c]   (tokens optional)
//   otherwise:     y[b, t, :] = tokens[b, t, :] = quiet NaN, no table row is read, *bad_ids = 1        (bad_ids optional)
//
// One rounded fp32 add of the same two operands as the chain's `tokens + pos`: the result equals it bit for bit.  The chain
// writes the [B, T, C] array three times (embedding, add, the one-element torch.cat) and reads it twice; this kernel
// stores every output element once.
//
// One workgroup (four waves) owns a strip of EM_TS consecutive tokens of one sample; the grid is the flat list of strips,
// sample slowest, so later samples find the position rows (and the whole table: 262 rows in the shipped model) in cache.
//   * wave = output row, lanes = that row's 16-byte vectors (V = 4: C, every pitch and sample stride multiples of 4, every
//     float pointer 16-byte aligned) or its dwords (V = 1: any 4-byte alignment); a wave instruction stores 1 KiB of a row.
//   * The id of a row is read once per row through a wave-uniform address (int32 or int64, range-tested at full width
//     before it indexes anything); the next row's id is fetched while this row streams.
//   * The flag is a plain store of the constant 1 by one lane of each wave that meets a bad id: every writer stores the same
//     value, nobody reads it here, the kernel never clears it.
//   * All offsets are 64-bit.  B * ceil(T / EM_TS) strips must fit a 31-bit grid (PIO_E_SHAPE otherwise).
//
// Stores are non-temporal (measured faster than plain ones: the note at em_store).
#include <type_traits>

#include "pio_internal.h"

namespace pio {

namespace {

constexpr int EM_TS = 32;  // tokens per strip

// Non-temporal stores ship: measured faster than plain stores on an MI355X alone (B = 100: 120 - 123 against 144 - 147 us,
// 5.2 against 4.3 TB/s; B = 8: 9.4 - 10.4 against 14.1 us; B = 1: 8.1 against 8.6 us), and never slower in the whole language
// step at B = 100, where the encoder's LayerNorm reads the array next (20.68 against 20.75 ms in one session, 20.84 against
// 20.84 ms in another; three alternating runs each, spreads up to 0.07 ms; profiles/language_front_end.json).
// -DPIO_EMBED_PLAIN builds the plain-store variant for A/B runs.
#ifdef PIO_EMBED_PLAIN
template <typename T>
__device__ __forceinline__ void em_store(T *p, T v) { *p = v; }
#else
template <typename T>
__device__ __forceinline__ void em_store(T *p, T v) { __builtin_nontemporal_store(v, p); }
#endif

struct EmbedArgs {
    const void *ids;
    const float *table, *pos;
    float *y, *tok;
    int32_t *bad;
    int64_t ids_sb, ldt, ldp, y_sb, ldy, tok_sb, ldtok;
    int32_t id_bytes, nV, T, C, strips;  // strips per sample
};

__device__ __forceinline__ int64_t em_load_id(const EmbedArgs &a, int64_t i) {
    return a.id_bytes == 8 ? static_cast<const int64_t *>(a.ids)[i] : (int64_t) static_cast<const int32_t *>(a.ids)[i];
}

// V = 4: rows leave as 16-byte vectors; V = 1: as dwords
template <int V>
__global__ __launch_bounds__(256) void embed_tokens_kernel(const EmbedArgs a) {
    using Vec = typename std::conditional<V == 4, f32x4, float>::type;
    const int b = blockIdx.x / a.strips, strip = blockIdx.x - b * a.strips;
    const int t0 = strip * EM_TS;
    const int n = min(EM_TS, a.T - t0);
    const int lane = threadIdx.x & 63, wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int nvec = a.C / V;  // (V = 4: C % 4 == 0)
    const int64_t idrow = (int64_t)b * a.ids_sb + t0;
    const float quiet_nan = __builtin_nanf("");

    int64_t id = wave < n ? em_load_id(a, idrow + wave) : 0;
    for (int r = wave; r < n; r += 4) {
        const int64_t next = r + 4 < n ? em_load_id(a, idrow + r + 4) : 0;
        const int64_t t = t0 + r;
        const bool ok = id >= 0 && id < (int64_t)a.nV;
        Vec *yrow = reinterpret_cast<Vec *>(a.y + (int64_t)b * a.y_sb + t * a.ldy);
        Vec *krow = a.tok ? reinterpret_cast<Vec *>(a.tok + (int64_t)b * a.tok_sb + t * a.ldtok) : nullptr;
        if (ok) {
            const Vec *erow = reinterpret_cast<const Vec *>(a.table + id * a.ldt);
            const Vec *prow = reinterpret_cast<const Vec *>(a.pos + t * a.ldp);
            for (int cv = lane; cv < nvec; cv += 64) {
                const Vec e = erow[cv], p = prow[cv];
                Vec o;
                if constexpr (V == 4) {
                    o = Vec{__fadd_rn(e[0], p[0]), __fadd_rn(e[1], p[1]), __fadd_rn(e[2], p[2]), __fadd_rn(e[3], p[3])};
                } else {
                    o = __fadd_rn(e, p);
                }
                em_store(yrow + cv, o);
                if (krow) em_store(krow + cv, e);
            }
        } else {
            Vec o;
            if constexpr (V == 4) {
                o = Vec{quiet_nan, quiet_nan, quiet_nan, quiet_nan};
            } else {
                o = quiet_nan;
            }
            for (int cv = lane; cv < nvec; cv += 64) {
                em_store(yrow + cv, o);
                if (krow) em_store(krow + cv, o);
            }
            if (a.bad && lane == 0) *a.bad = 1;
        }
        id = next;
    }
}

// true when rows * ld (rows >= 1, ld >= 0) exceeds `have`, without overflowing
inline bool em_short(int64_t have, int64_t rows, int64_t ld) { return ld > INT64_MAX / rows || have < rows * ld; }

}  // namespace

int embed_tokens_launch(const void *ids, int id_bytes, int64_t ids_sb, const float *table, int64_t ldt, int V,
                        const float *pos, int64_t ldp, float *y, int64_t y_sb, int64_t ldy, float *tokens, int64_t tok_sb,
                        int64_t ldtok, int32_t *bad_ids, int B, int T, int C, hipStream_t s) {
    if (!ids || !table || !pos || !y) return PIO_E_ARG;
    if (id_bytes != 4 && id_bytes != 8) return PIO_E_ARG;
    if ((uintptr_t)ids & (uintptr_t)(id_bytes - 1)) return PIO_E_ARG;
    if (((uintptr_t)table | (uintptr_t)pos | (uintptr_t)y | (uintptr_t)tokens | (uintptr_t)bad_ids) & 3) return PIO_E_ARG;
    if (B < 1 || T < 1 || C < 1 || V < 1) return PIO_E_SHAPE;
    if (ldt < C || ldp < C || ldy < C || (tokens && ldtok < C)) return PIO_E_SHAPE;
    if (B > 1 && (ids_sb < T || em_short(y_sb, T, ldy) || (tokens && em_short(tok_sb, T, ldtok)))) return PIO_E_SHAPE;
    if (tokens == y) return PIO_E_SHAPE;
    const int64_t strips = ((int64_t)T + EM_TS - 1) / EM_TS;
    if (strips * B > 0x7fffffffLL) return PIO_E_SHAPE;
    bool vec = C % 4 == 0 && ldt % 4 == 0 && ldp % 4 == 0 && ldy % 4 == 0 && (B == 1 || y_sb % 4 == 0) &&
               !(((uintptr_t)table | (uintptr_t)pos | (uintptr_t)y) & 15);
    if (tokens) vec = vec && ldtok % 4 == 0 && (B == 1 || tok_sb % 4 == 0) && !((uintptr_t)tokens & 15);
    EmbedArgs a;
    a.ids = ids, a.table = table, a.pos = pos, a.y = y, a.tok = tokens, a.bad = bad_ids;
    a.ids_sb = B > 1 ? ids_sb : 0, a.ldt = ldt, a.ldp = ldp, a.y_sb = B > 1 ? y_sb : 0, a.ldy = ldy;
    a.tok_sb = B > 1 ? tok_sb : 0, a.ldtok = ldtok;
    a.id_bytes = id_bytes, a.nV = V, a.T = T, a.C = C, a.strips = (int32_t)strips;
    const double out = 4.0 * B * T * (double)C;
    ProfScope prof(PROF_LAYERNORM, 0.0, out * (tokens ? 2.0 : 1.0) + 4.0 * T * (double)C + (double)id_bytes * B * T, s);
    const dim3 grid((unsigned)(strips * B));
    if (vec)
        hipLaunchKernelGGL(embed_tokens_kernel<4>, grid, dim3(256), 0, s, a);
    else
        hipLaunchKernelGGL(embed_tokens_kernel<1>, grid, dim3(256), 0, s, a);
    return launch_status();
}

}  // namespace pio
