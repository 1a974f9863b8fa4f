// balance.hip -- a train epoch's class-balanced visit order, drawn on the device (iterator_train__balance).
//
// The reference balances its dataset once, before any split (helper.py:355-388): under-sample the large classes without
// replacement, over-sample the small ones with replacement, targets smoothed around the mean class size
// (slnlp/balance.py: sampling_targets).  Here the same targets are applied to ONE FIT'S TRAIN SPLIT, afresh every epoch, and the
// result goes straight into the order table the gather launches read -- no host order crosses the bus.
//
// The draw (tests/balance_ref.py is its numpy restatement; include/slnlp.h states it for callers): labels y [n], class c with
// n_c rows keeps u_c and is visited t_c times, n_bal = sum t_c.  Random words are Threefry-4x32 (the dropout masks' rounds) under
// key (seed_lo, seed_hi, 0, 0) at counter (index, epoch, stage, 0); a 64-bit key is X1 << 32 | X0, the over-sampling word X0.
//   stage 0, index = row i:        rows of a class ranked by (key, i); the u_c lowest are kept, kept_c[r] = row of rank r
//   stage 1, index = base_c + j:   extra j of class c (j < t_c - u_c, base_c = the class's first slot) takes kept_c[mulhi32(X0, u_c)]
//   stage 2, index = slot:         the slots -- class after class, kept rows then extras -- ranked by (key, slot); order[rank] = row
// Every rank is a count of smaller (key, index) pairs: a pure function of the inputs, whatever the grid or the waves' timing.
// No atomics, no lists built by arrival.  Two launches: the first ranks the rows within their classes and stores the stage-2
// keys, the second fills the slots and ranks them.  The counting is quadratic (n_c^2 per class, n_bal^2 / 4 per wave of the
// shuffle), which is why a plan refuses more than SLNLP_BALANCE_MAX_ROWS rows; at a few thousand rows it is microseconds.
#include <math.h>

#include <algorithm>
#include <vector>

#include "common.hpp"
#include "launch.hpp"

// per class (present classes only, ascending id), 6 ints each
enum { BC_COUNT = 0, BC_KEEP = 1, BC_VISIT = 2, BC_BASE = 3, BC_MEMBERS = 4, BC_KEPT = 5, BC_FIELDS = 6 };

struct slnlp_balance_plan {
    int64_t n = 0, n_bal = 0;
    int n_present = 0, n_kept = 0;
    std::vector<int> host;                  // the upload's source, alive as long as the tables
    char* dev = nullptr;                    // one allocation: the tables below, then the two scratch arrays
    const int* cls = nullptr;               // [n_present, BC_FIELDS]
    const int* members = nullptr;           // [n] rows, class after class, ascending within a class
    const int* member_cls = nullptr;        // [n] index (into cls) of the class of members[p]
    const int* slot_cls = nullptr;          // [n_bal] index of the class of slot s
    int* kept = nullptr;                    // scratch [n_kept]: kept_c[r] at cls[c].kept + r      (launch 1 -> launch 2)
    unsigned long long* key2 = nullptr;     // scratch [n_bal]: the slots' stage-2 keys              (launch 1 -> launch 2)
};

namespace slnlp {

__device__ __forceinline__ unsigned long long balance_key64(unsigned index, unsigned stage, const SeedKey& K) {
    const uint4 w = seed_words(index, stage, K);
    return ((unsigned long long)w.y << 32) | w.x;
}

// Launch 1.  Blocks [0, rank_blocks): thread p takes members[p] = row i of class c, counts the class's rows with a smaller
// (stage-0 key, row) and, when that rank is below u_c, stores i as kept_c[rank].  members lists a class's rows together, so
// the classes of a block's 256 rows cover ONE range of member positions: the block walks that range 256 positions at a time,
// every thread draws one key of the tile into LDS, and each thread compares the part of the tile that is its own class
// (a key costs ~100 instructions, a comparison a handful: drawn once per block, not once per pair).
// Blocks from rank_blocks on: the stage-2 key of every slot.
__device__ __forceinline__ void balance_rank_body(const int* __restrict__ cls, const int* __restrict__ members,
                                                  const int* __restrict__ member_cls, int n, int n_bal, int rank_blocks,
                                                  unsigned long long seed, unsigned epoch, int* __restrict__ kept,
                                                  unsigned long long* __restrict__ key2) {
    __shared__ unsigned long long tile_key[256];
    __shared__ int tile_row[256];
    const SeedKey K = seed_key(seed, epoch);
    if ((int)blockIdx.x >= rank_blocks) {
        const int s = ((int)blockIdx.x - rank_blocks) * 256 + (int)threadIdx.x;
        if (s < n_bal) key2[s] = balance_key64((unsigned)s, 2u, K);
        return;
    }
    const int p0 = (int)blockIdx.x * 256, p = p0 + (int)threadIdx.x;
    const bool live = p < n;
    // the member positions the block's classes cover: from the first class's first row to the last class's last
    const int* c_lo = cls + member_cls[p0] * BC_FIELDS;
    const int* c_hi = cls + member_cls[min(p0 + 255, n - 1)] * BC_FIELDS;
    const int lo = c_lo[BC_MEMBERS], hi = c_hi[BC_MEMBERS] + c_hi[BC_COUNT];
    const int* c = cls + member_cls[live ? p : p0] * BC_FIELDS;
    const int i = live ? members[p] : 0;
    const int first = live ? c[BC_MEMBERS] : 0, end = live ? first + c[BC_COUNT] : 0;      // (a thread past n compares nothing)
    const unsigned long long mine = balance_key64((unsigned)i, 0u, K);
    int rank = 0;
    for (int t0 = lo; t0 < hi; t0 += 256) {
        const int src = t0 + (int)threadIdx.x;
        __syncthreads();                                 // the previous tile has been read
        if (src < hi) {
            const int m = members[src];
            tile_row[threadIdx.x] = m;
            tile_key[threadIdx.x] = balance_key64((unsigned)m, 0u, K);
        }
        __syncthreads();
        const int q1 = min(end, min(hi, t0 + 256)) - t0;
        for (int q = max(first, t0) - t0; q < q1; ++q) {
            const unsigned long long other = tile_key[q];
            rank += (other < mine || (other == mine && tile_row[q] < i)) ? 1 : 0;
        }
    }
    // (a class that keeps all its rows is ranked too: kept_c is the class in rank order, which the over-sampling draws index)
    if (live && rank < c[BC_KEEP]) kept[c[BC_KEPT] + rank] = i;
}
SLNLP_ZKERNEL(balance_rank_kernel, 256, balance_rank_body)

// Launch 2.  A block owns 64 consecutive slots; lane l of every wave stands for slot 64 * block + l.  The stage-2 keys pass
// through LDS 256 at a time and wave w compares its quarter of each tile, so a slot's rank is the sum of four partial counts
// (integers: any order gives the same sum).  Wave 0 then looks the slot's row up and stores order[rank] (and the label).
__device__ __forceinline__ void balance_fill_body(const int* __restrict__ cls, const int* __restrict__ slot_cls,
                                                  const int* __restrict__ kept, const unsigned long long* __restrict__ key2, int n_bal,
                                                  unsigned long long seed, unsigned epoch, const int64_t* __restrict__ y,
                                                  int64_t* __restrict__ order, int64_t* __restrict__ y_out) {
    __shared__ unsigned long long tile[256];
    __shared__ int part[4][64];
    const int lane = (int)threadIdx.x & 63, wave = (int)threadIdx.x >> 6;
    const int s = (int)blockIdx.x * 64 + lane;
    const bool live = s < n_bal;
    const unsigned long long mine = live ? key2[s] : 0ull;
    int rank = 0;
    for (int t0 = 0; t0 < n_bal; t0 += 256) {
        const int src = t0 + (int)threadIdx.x;
        __syncthreads();                                 // the previous tile has been read
        tile[threadIdx.x] = src < n_bal ? key2[src] : 0ull;
        __syncthreads();
        const int q0 = wave * 64;
        const int q1 = min(q0 + 64, n_bal - t0);         // (entries past n_bal are not slots)
        for (int q = q0; q < q1; ++q) {
            const unsigned long long other = tile[q];    // one address for the whole wave: a broadcast read
            rank += (other < mine || (other == mine && t0 + q < s)) ? 1 : 0;
        }
    }
    part[wave][lane] = rank;
    __syncthreads();
    if (wave != 0 || !live) return;
    rank = part[0][lane] + part[1][lane] + part[2][lane] + part[3][lane];
    const int* c = cls + slot_cls[s] * BC_FIELDS;
    const int j = s - c[BC_BASE], keep = c[BC_KEEP];
    int r = j;
    if (j >= keep) {
        const SeedKey K = seed_key(seed, epoch);
        const unsigned w = seed_words((unsigned)(c[BC_BASE] + (j - keep)), 1u, K).x;
        r = (int)(((unsigned long long)w * (unsigned)keep) >> 32);           // mulhi32: in [0, keep)
    }
    const int row = kept[c[BC_KEPT] + r];
    order[rank] = row;                                   // rank in [0, n_bal): the count of n_bal - 1 other slots at most
    if (y_out) y_out[rank] = y[row];
}
SLNLP_ZKERNEL(balance_fill_kernel, 256, balance_fill_body)

static int round_half_even(double v) { return (int)nearbyint(v); }       // Python's round() (the default rounding mode)

static void balance_plan_destroy(slnlp_balance_plan* bp) {
    if (!bp) return;
    if (bp->dev) (void)hipFree(bp->dev);
    delete bp;
}

static int balance_plan_create(const int64_t* y, int64_t n, int n_classes, hipStream_t st, slnlp_balance_plan** out) {
    SLNLP_CHECK_ARG(out, "balance_plan_create: null out");
    *out = nullptr;
    SLNLP_CHECK_ARG(y, "balance_plan_create: null labels");
    SLNLP_CHECK_ARG(n >= 1 && n <= SLNLP_BALANCE_MAX_ROWS, "balance_plan_create: n=%ld outside 1..%d", (long)n, SLNLP_BALANCE_MAX_ROWS);
    SLNLP_CHECK_ARG(n_classes >= 1, "balance_plan_create: n_classes=%d", n_classes);
    std::vector<int> count((size_t)n_classes, 0);
    for (int64_t i = 0; i < n; ++i) {
        SLNLP_CHECK_ARG(y[i] >= 0 && y[i] < n_classes, "balance_plan_create: label %ld of row %ld outside [0, %d)", (long)y[i], (long)i,
                        n_classes);
        ++count[(size_t)y[i]];
    }
    int present = 0;
    for (int c = 0; c < n_classes; ++c) present += count[c] > 0;
    // slnlp/balance.py sampling_targets, in the same double arithmetic: u = n / classes present, smooth(v) = round(u + ln v),
    // under = min(n_c, smooth(n_c)), over = max(under, smooth(under))
    const double u = (double)n / (double)present;
    std::vector<int> cls((size_t)present * BC_FIELDS), index_of((size_t)n_classes, -1);
    int64_t slots = 0, kept = 0;
    int members = 0, k = 0;
    for (int c = 0; c < n_classes; ++c) {
        if (!count[c]) continue;
        const int under = std::min(count[c], round_half_even(u + log((double)count[c])));
        const int over = std::max(under, round_half_even(u + log((double)under)));
        SLNLP_CHECK_ARG(under >= 1, "balance_plan_create: class %d keeps %d rows", c, under);
        int* e = &cls[(size_t)k * BC_FIELDS];
        e[BC_COUNT] = count[c]; e[BC_KEEP] = under; e[BC_VISIT] = over;
        e[BC_BASE] = (int)slots; e[BC_MEMBERS] = members; e[BC_KEPT] = (int)kept;
        index_of[c] = k++;
        slots += over; kept += under; members += count[c];
        SLNLP_CHECK_ARG(slots <= SLNLP_BALANCE_MAX_ROWS, "balance_plan_create: a balanced epoch of more than %d rows (the order-table limit)",
                        SLNLP_BALANCE_MAX_ROWS);
    }
    slnlp_balance_plan* bp = new slnlp_balance_plan;
    bp->n = n; bp->n_bal = slots; bp->n_present = present; bp->n_kept = (int)kept;
    // host image: cls | members | member_cls | slot_cls
    const size_t o_members = cls.size(), o_mcls = o_members + (size_t)n, o_scls = o_mcls + (size_t)n, ints = o_scls + (size_t)slots;
    bp->host.resize(ints);
    std::copy(cls.begin(), cls.end(), bp->host.begin());
    std::vector<int> fill((size_t)present);
    for (int j = 0; j < present; ++j) fill[j] = cls[(size_t)j * BC_FIELDS + BC_MEMBERS];
    for (int64_t i = 0; i < n; ++i) {                    // rows in ascending order within every class
        const int j = index_of[(size_t)y[i]];
        bp->host[o_members + fill[j]] = (int)i;
        bp->host[o_mcls + fill[j]] = j;
        ++fill[j];
    }
    for (int j = 0; j < present; ++j) {
        const int* e = &cls[(size_t)j * BC_FIELDS];
        std::fill_n(bp->host.begin() + o_scls + e[BC_BASE], e[BC_VISIT], j);
    }
    const size_t table_bytes = (ints * sizeof(int) + 15) / 16 * 16;
    const size_t key_bytes = (size_t)slots * sizeof(unsigned long long);
    const size_t bytes = table_bytes + key_bytes + (size_t)kept * sizeof(int);
    if (hipMalloc(&bp->dev, bytes) != hipSuccess ||
        hipMemcpyAsync(bp->dev, bp->host.data(), ints * sizeof(int), hipMemcpyHostToDevice, st) != hipSuccess) {
        set_error("balance_plan_create: allocating / uploading the tables failed: %s", hipGetErrorString(hipGetLastError()));
        balance_plan_destroy(bp);
        return SLNLP_ERR_LAUNCH;
    }
    const int* base = reinterpret_cast<const int*>(bp->dev);
    bp->cls = base; bp->members = base + o_members; bp->member_cls = base + o_mcls; bp->slot_cls = base + o_scls;
    bp->key2 = reinterpret_cast<unsigned long long*>(bp->dev + table_bytes);
    bp->kept = reinterpret_cast<int*>(bp->dev + table_bytes + key_bytes);
    *out = bp;
    return 0;
}

static int balanced_order(const slnlp_balance_plan* bp, const int64_t* y_dev, uint64_t seed, int64_t epoch, int64_t* order_out,
                          int64_t* y_out, hipStream_t st) {
    SLNLP_CHECK_ARG(bp && order_out, "balanced_order: null plan or order_out");
    SLNLP_CHECK_ARG(y_dev || !y_out, "balanced_order: y_out needs the device labels");
    SLNLP_CHECK_ARG(epoch >= 0 && epoch <= 0xffffffffLL, "balanced_order: epoch %ld outside [0, 2^32)", (long)epoch);
    const int n = (int)bp->n, n_bal = (int)bp->n_bal;
    const int rank_blocks = ceil_div(n, 256);
    SLNLP_TRY(zlaunch(balance_rank_kernel, dim3(rank_blocks + ceil_div(n_bal, 256)), 256, 0, st, "balance_rank", bp->cls, bp->members,
                      bp->member_cls, n, n_bal, rank_blocks, (unsigned long long)seed, (unsigned)epoch, bp->kept, bp->key2));
    return zlaunch(balance_fill_kernel, dim3(ceil_div(n_bal, 64)), 256, 0, st, "balance_fill", bp->cls, bp->slot_cls, (const int*)bp->kept,
                   (const unsigned long long*)bp->key2, n_bal, (unsigned long long)seed, (unsigned)epoch, y_dev, order_out, y_out);
}

}  // namespace slnlp

extern "C" {
int slnlp_balance_plan_create(const int64_t* y_host, int64_t n, int n_classes, void* stream, slnlp_balance_plan** out) {
    return slnlp::balance_plan_create(y_host, n, n_classes, (hipStream_t)stream, out);
}
int64_t slnlp_balance_plan_rows(const slnlp_balance_plan* plan) { return plan ? plan->n_bal : -1; }
void slnlp_balance_plan_destroy(slnlp_balance_plan* plan) { slnlp::balance_plan_destroy(plan); }
int slnlp_balanced_order(const slnlp_balance_plan* plan, const int64_t* y_dev, uint64_t seed, int64_t epoch, int64_t* order_out,
                         int64_t* y_out, void* stream) {
    return slnlp::balanced_order(plan, y_dev, seed, epoch, order_out, y_out, (hipStream_t)stream);
}
}
