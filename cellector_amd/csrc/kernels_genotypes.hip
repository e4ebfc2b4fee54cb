// cellector_class_genotypes: the K-class allele tallies over ALL loci (also those failing min_ref / min_alt), one pass over the staged
// COO whatever K.  load_mtx_final (load_data.rs:109-132) re-reads both matrices for its two classes; k_final_tallies
// (kernels_em.hip) is that pass for the exclusion set against the rest; this is the pass for a labelling with up to 16 classes.  The
// genotype rule over the tallies runs on the host (genotype_host.h).
//
// acc = [K + 1][2][total_loci] u64: per slot the alt plane, then the ref plane; slot K collects the cells labelled 255.  Sums of
// integers added with 64-bit atomics: exact and independent of the order the hardware performs them in, and of the order of the
// entries (file order after an ingest, ascending after a combine, arbitrary after cellector_ingest_coo).
#include "ctx.h"
#include "device_math.h"

#define GT_THREADS 256
#define GT_SLOT_BITS 5  // slot <= 16

// One entry per lane.  A lane's destination is key = (locus, slot); its two counts travel as one word, alt in the low half and ref
// in the high half: a wave's 64 x 65535 stays below 2^32, so one reduction serves both alleles without a carry between the halves.
// The wave peels its distinct keys one per round: the first unfinished lane's key is broadcast, the lanes that carry it are summed
// (the others contribute 0), lane 0 issues at most two atomics, and the selected lanes retire.  The loop condition is a ballot,
// hence wave-uniform: every lane of the wave runs every round, which the shuffles inside need.  Locus-major input (a wave inside
// one locus) takes as many rounds as slots are present; 64 distinct keys take 64 rounds.  An entry with alt = ref = 0 adds
// nothing and never opens a round.
__global__ __launch_bounds__(GT_THREADS) void k_genotype_tallies(uint64_t n, uint64_t total_loci, uint64_t n_cells, uint32_t K,
                                                                 const uint32_t *__restrict__ locus, const uint32_t *__restrict__ cell,
                                                                 const uint16_t *__restrict__ alt, const uint16_t *__restrict__ ref,
                                                                 const uint8_t *__restrict__ lab, unsigned long long *__restrict__ acc)
{
    const uint64_t i = (uint64_t)blockIdx.x * GT_THREADS + threadIdx.x;
    const int lane = threadIdx.x & 63;
    uint64_t key = ~0ull, packed = 0;
    if (i < n) {
        const uint64_t l = locus[i], c = cell[i];
        if (l < total_loci && c < n_cells) {  // (the staged COO holds no other entry; nothing is written outside acc in any case)
            const uint32_t lb = lab[c];
            key = l << GT_SLOT_BITS | (lb < K ? lb : K);
            packed = (uint64_t)alt[i] | (uint64_t)ref[i] << 32;
        }
    }
    unsigned long long todo = __ballot(packed != 0);
    while (todo) {
        const int src = __ffsll((long long)todo) - 1;
        const uint64_t k0 = (uint64_t)__shfl((long long)key, src, 64);
        const bool mine = key == k0;
        const uint64_t s = wave_sum_u64(mine ? packed : 0ull);  // (valid in lane 0, which every wave of the grid has)
        if (lane == 0) {
            unsigned long long *const pa = acc + (k0 & ((1u << GT_SLOT_BITS) - 1)) * 2 * total_loci + (k0 >> GT_SLOT_BITS);
            const unsigned long long a = s & 0xffffffffull, r = s >> 32;
            if (a) atomicAdd(pa, a);
            if (r) atomicAdd(pa + total_loci, r);
        }
        todo &= ~__ballot(mine);
    }
}

cellector_status launch_genotype_tallies(cellector_ctx *c, const uint8_t *d_lab, uint32_t K, uint64_t *d_acc)
{
    const uint64_t n = c->coo.n;
    const uint64_t grid = (n + GT_THREADS - 1) / GT_THREADS;
    if (grid > 0x7fffffffull)
        return ctx_fail(c, CELLECTOR_EINVAL, "class_genotypes: %llu staged entries, one launch covers below 2^39", (unsigned long long)n);
    HIPCHK(c, hipMemsetAsync(d_acc, 0, (uint64_t)(K + 1) * 2 * c->total_loci * 8, c->stream));
    if (n) {
        hipLaunchKernelGGL(k_genotype_tallies, dim3((unsigned)grid), dim3(GT_THREADS), 0, c->stream, n, c->total_loci, c->nloc, K,
                           c->coo.locus.get(), c->coo.cell.get(), c->coo.alt.get(), c->coo.ref.get(), d_lab,
                           (unsigned long long *)d_acc);
    }
    HIPCHK(c, hipGetLastError());
    return CELLECTOR_OK;
}
