/*
 * grpath_synth.h — synthetic ONT-like read generator on the GPU (measurement
 * support for bench.py; not part of the reference's path and not used by the
 * goldrush-path CLI).  Exported by libgrpath_hip.so.
 *
 * Model: uniform random genome of `genome_len` bases defined
 * by a counter-based generator (base i = f(genome_seed, i); optionally repeat-rich,
 * repeat_frac below); read r is the
 * substring starting at start[r] (genome coordinates wrap), reverse-
 * complemented when strand[r] != 0, passed through i.i.d. errors: each source
 * base is deleted with probability p_del, otherwise emitted (substituted by a
 * different base with probability p_sub) and followed by one random inserted
 * base with probability p_ins.  Exactly len[r] bases are produced per read and
 * written 2-bit packed (grpath.h encoding) at word_off[r]: (len[r] + 15) / 16
 * words, the bits behind the last base zero, and no other word of the output.
 * On the other strand the source is walked downwards from start[r] (which is
 * its first base, complemented), wrapping below 0.  A read of more bases than
 * the genome walks round it again.  An insertion that the end of the read leaves
 * no room for is dropped.
 *
 * The errors of a read are a function of error_seed, of the read's index r
 * INSIDE THE CALL and of the source base's index inside the read, and of
 * nothing else: the same plan cut into other batches gives other reads, and read
 * j of every batch of a run has the same error pattern (the same source bases
 * deleted, substituted, followed by an insertion) as read j of every other batch.
 * Genome, start, length and strand do not enter it.
 *
 * Accepted ranges (anything else is refused with -1 before the device is
 * touched; grp_synth_last_error says why):
 *   genome_len     1 .. 2^63
 *   p_sub, p_ins   finite, 0 .. 1.  A probability acts as the 20-bit threshold
 *                  (uint32)(p * 2^20): below 2^-20 it is 0, and 1 is "always".
 *   p_del          finite, >= 0 and (uint32)(p_del * 2^20) < 2^20, i.e. below 1:
 *                  a read of deleted bases alone would never be complete.  The
 *                  cost of a read grows as 1 / (1 - p_del).
 *   repeat_frac    finite, >= 0; 1.5 * repeat_frac is clamped to 1, so from 2/3
 *                  on every slot is a repeat copy.
 * tests/synth_model.py restates the model on the host; the kernel is held to it
 * bit for bit (tests/test_gpu_synth.py).
 */
#ifndef GRPATH_SYNTH_H
#define GRPATH_SYNTH_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct
{
  uint64_t genome_len;
  uint64_t genome_seed;
  uint64_t error_seed;
  float p_sub, p_ins, p_del;
  /* Round 5: the share of the genome made of REPEATS, 0 = none (the uniform genome of rounds
   * 1-4: two reads share k-mers only where they overlap).  With f > 0 the genome is cut into slots of 6144 bases; a
   * slot is a repeat copy with probability 1.5 f and then begins with its family's unit — 2 to 6 kb long (per family),
   * the family's consensus with a copy-specific substitution at 1 to 5 % of the positions (per family) — the rest of
   * the slot and every other slot are unique sequence.  Families come in three tiers of ~10 000, ~1 000 and ~30 copies
   * (a third of the repeat slots each; fewer copies where the genome is too small for that many). */
  float repeat_frac;
} grp_synth_params;

/*
 * d_packed_out: device memory of word_off[n_reads] 32-bit words (caller
 * allocates; e.g. a torch tensor or grp_synth_alloc).  start / len / strand /
 * word_off are HOST arrays (word_off of n_reads + 1 entries; read r is written
 * at word_off[r], wherever the caller put it).  `stream` is a hipStream_t (NULL
 * = default stream); the call returns after the kernel has completed.  Returns 0
 * on success, -1 for an argument outside the accepted ranges (nothing was
 * written), -3 for a HIP error; the device arrays of the call are released on
 * every return.
 */
int grp_synth_reads(const grp_synth_params* p,
                    const uint64_t* start,
                    const uint32_t* len,
                    const uint8_t* strand,
                    const uint64_t* word_off,
                    uint32_t n_reads,
                    void* d_packed_out,
                    void* stream);

/* plain hipMalloc / hipFree / device->host copy, for callers without torch */
void* grp_synth_alloc(uint64_t bytes);
void grp_synth_free(void* d);
int grp_synth_download(const void* d, uint64_t bytes, void* host);
const char* grp_synth_last_error(void);

#ifdef __cplusplus
}
#endif
#endif
