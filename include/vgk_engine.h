/*
 * vgk_engine.h — entry points of the ENGINE library (vg_amd/libvgamd.so) that the CPU oracle has no counterpart for.
 *
 * include/vgk.h is the ABI both libraries export, symbol for symbol; what is declared here exists in the engine library only: calls whose
 * reference is not the oracle but a restatement elsewhere in the tree, and counters of the engine's own machinery.  Types, error codes and
 * conventions are vgk.h's (return 0 = VGK_OK, < 0 = VGK_E*; plain pointers and sizes; no exception crosses the boundary); vgk_abi_version()
 * is not touched by additions here.
 *
 * ---- find_seeds' choice on the device, for reads of any length ---------------------------------------------------------------------------
 * vgk.h's vgk_minimizer_list / vgk_minimizer_seeds_of leave MinimizerMapper::find_seeds' choice of minimizers (src/minimizer_mapper.cpp:4109-4440)
 * to the caller between them.  The two calls below make it on the device, by exactly the rule of the host shim's select_minimizers
 * (vg_amd/host/seed_policy.cpp:55-193), for any number of minimizers per read: find_minimizers' scores (1 + ln(hard_hit_cap) - ln(hits), 1 beyond
 * the hard cap, 0 without hits — the logarithms taken once on the host), the order (score descending, key, read position), the runs that share the
 * best score shuffled as sort_shuffling_ties shuffles them (Knuth's shuffle over std::minstd_rand seeded from the read's bytes — THE BYTES THE CALLER
 * GIVES: lower case and N included, nothing is masked, and no read is ever handed back to the host), window downsampling (sample_minimal), and
 * the filters in score order, run by run: downsampled, no hits, the run's hits beyond the hard cap, exclude-overlapping, the unique-minimizer
 * budget (max_unique_min / num_bp_per_min / minimizer_coverage_flank), the score fraction.  Single-end rule: one generator per read.
 *
 * A C caller that maps long reads needs nothing but
 *     vgk_create -> vgk_minimizer_index_create -> vgk_minimizer_find_seeds (sizes unknown: call with cap_m = cap_s = 0, read written[0..1] off
 *     VGK_EOPS, allocate, call again)
 * and gets, per read, its minimizers, which of them were taken, and the seeds of those.
 */
#ifndef VGK_ENGINE_H
#define VGK_ENGINE_H
#include "vgk.h"
#ifdef __cplusplus
extern "C" {
#endif

/* MinimizerMapper's fields of the same names (src/minimizer_mapper.hpp:140-260).  0 switches off: hit_cap (with minimizer_score_fraction 1.0:
 * the score filter), max_unique_min (the budget), num_bp_per_min (its read-length term), exclude_overlapping_min, minimizer_downsampling_window_count.
 * The downsampling window of a read of L bases is min(L / window_count, max_window_length), none when L < window_count * k. */
typedef struct vgk_find_seeds_policy {
    uint32_t hit_cap, hard_hit_cap;  double minimizer_score_fraction;
    uint32_t max_unique_min, num_bp_per_min, minimizer_coverage_flank, exclude_overlapping_min;
    uint32_t minimizer_downsampling_window_count, reserved;  uint64_t minimizer_downsampling_max_window_length;
} vgk_find_seeds_policy;

/* The filter that dropped a minimizer (SeedFilter of vg_amd/host/seed_policy.hpp); 0 = its hits become seeds */
#define VGK_SEED_TAKEN        0
#define VGK_SEED_DOWNSAMPLED  1
#define VGK_SEED_NO_HITS      2
#define VGK_SEED_HARD_HIT_CAP 3
#define VGK_SEED_OVERLAPPING  4
#define VGK_SEED_MAX_MIN      5
#define VGK_SEED_HIT_CAP      6

/* The choice alone, over a list as vgk_minimizer_list answers it — any list: no index is needed.  Read r is reads[read_off[r] .. read_off[r + 1]),
 * its minimizers are minimizers[minimizer_off[r] .. minimizer_off[r + 1]) in order of read offset, each k bases long (key, offset, hits are read;
 * flags are not).  verdict[j] (one byte per minimizer): VGK_SEED_*.
 * VGK_EINVAL: hard_hit_cap 0 or above 65535; a fraction outside [0, 1]; a minimizer that does not fit its read (offset + k > read length) or
 * lies before its predecessor; a read whose downsampling window is shorter than k (the reference stops there). */
int vgk_minimizer_choose(vgk_ctx* ctx, const vgk_find_seeds_policy* policy, uint32_t k, const char* reads, const uint64_t* read_off, uint32_t n,
                         const uint64_t* minimizer_off, const vgk_read_minimizer* minimizers, uint8_t* verdict);

/* List -> choice -> the seeds of the taken, in one call: the list and the choice stay in HBM between the three groups of kernels.  Outputs as
 * those of vgk_minimizer_list, the caller's choice and vgk_minimizer_seeds_of: minimizer_off[n + 1]; minimizers and take (1 = taken) up to cap_m;
 * seed_off[n_minimizers + 1] (room for cap_m + 1) and seeds up to cap_s.  VGK_EOPS when cap_m or cap_s is too small, with written[0] = the
 * minimizers and written[1] = the seeds there are — both from one call, whichever was short: the list is made in HBM whatever room the caller has. */
int vgk_minimizer_find_seeds(vgk_ctx* ctx, const vgk_minimizer_index* index, const vgk_find_seeds_policy* policy, const char* reads, const uint64_t* read_off, uint32_t n,
                             uint64_t* minimizer_off, vgk_read_minimizer* minimizers, uint8_t* take, size_t cap_m,
                             uint64_t* seed_off, vgk_seed* seeds, size_t cap_s, size_t written[2]);

/* Device time (ms) of the choice kernels of the last vgk_minimizer_choose / vgk_minimizer_find_seeds call on this context */
double vgk_minimizer_choose_last_ms(vgk_ctx* ctx);

/* ---- the speculative fill's counters ------------------------------------------------------------------------------------------------------
 * What the second fill of the last speculative run of a resident gssw batch did, read back from the device after the run (for tests and
 * measurements): out[0] = wavefronts filled a second time, out[1] = their steps summed, out[2] = reads on the miss list, out[3] = of those, reads
 * whose second fill began right of column 0, out[4] = walks that asked for a code left of where it began (must be 0).  All 0 when the last run
 * did not speculate ("speculation with feedback"). */
int vgk_batch_refill_stats(vgk_batch* batch, uint64_t out[5]);

/* The constant the rows of this batch's speculative first fill carry (the offset form of the rows), pre-multiplied by the score scale;
 * 0 when the batch does not speculate or that fill runs the saturating rows (the scoring leaves no room for a constant, or VGAMD_NO_OFFSET_ROWS was set
 * when the batch was packed). */
uint32_t vgk_batch_row_offset(vgk_batch* batch);

/* ---- chaining anchors on the device: algorithms::find_best_chains over given transitions ---------------------------------------------------
 * The step between the seeds and the chain stage (src/algorithms/chain_items.cpp:735-877, called once per zip-code tree per read at
 * src/minimizer_mapper_from_chains.cpp:1646): the DP chain_items_dp (:385-648) over the transitions add_transition_if_legal lets through
 * (:270-355), the multi-chain traceback (:650-733) and the recombination positions of every chain (:793-868) — for thousands of (read, tree)
 * problems per call.  No distance index is needed: what reaches the DP in the reference is a list of (from, to, graph distance) — that list is
 * this call's input, in any order.  The rule is the host shim's find_best_chains (vg_amd/host/chain_items.cpp), result for result.
 *
 * A problem is its anchors in the order sort_anchor_indexes leaves them (read start ascending, read end descending) and its candidate
 * transitions.  Problem p's anchors are anchors[anchor_off[p] .. anchor_off[p + 1]), its candidates candidates[cand_off[p] .. cand_off[p + 1]);
 * `from` and `to` number the anchors within the problem.
 *
 * Out: problem p's chains are chains[chain_off[p] .. chain_off[p + 1]), best first (at least one: a problem without anchors, or max_chains 0,
 * has the reference's one empty chain of score 0).  A chain's anchors, left to right, are items[item_begin .. item_begin + n_items); the anchors
 * that introduce a recombination (rec_positions) are rec_right[rec_begin .. rec_begin + n_rec), the left boundaries of the backward pass
 * rec_left[rec_begin .. rec_begin + n_rec_left), both in chain order — the reference's rec_intervals exist exactly when n_rec_left == n_rec.
 * Room, all the caller's: chain_off n_problems + 1; chains the sum over the problems of max(1, min(anchors, max_chains)); items, rec_right,
 * rec_left the number of anchors each (at least 1).  table_score / table_source (nullable, one entry per anchor): the DP table, source
 * UINT32_MAX = from nowhere.
 *
 * Ties the reference leaves to std::sort are fixed here [PARITY-UNPINNED]: traceback starts by score descending, then source descending
 * (nowhere largest), then anchor number ascending; chains by penalty ascending, then in order of creation.
 *
 * VGK_EINVAL: anchors out of order or of length 0; from / to outside the problem; a negative recombination_penalty or consistency_bonus; a
 * gap_scale that is negative or not finite; offsets that do not ascend (or do not begin at 0).  VGK_EUNSUPPORTED: an indel limit above
 * vgk_chain_items_limits' out[1]; a problem whose score sums could leave int32.  VGK_ETOOBIG: more than 2^32 - 16 anchors or candidates. */
typedef struct vgk_chain_anchor {      /* 48 B; algorithms::Anchor without its positions and zip codes */
    uint32_t read_start, length, margin_before, margin_after;
    int32_t  score;  uint32_t start_hint_offset, end_hint_offset, base_seed_length;
    uint64_t start_paths, end_paths;
} vgk_chain_anchor;
/* anchor numbers within the problem; the distance between the two hint points, as ZipCodeTree::find_distances reports it */
typedef struct vgk_chain_candidate { uint32_t from, to, graph_distance; } vgk_chain_candidate;
typedef struct vgk_chain_scheme {
    int32_t item_bonus, recombination_penalty, consistency_bonus;  uint32_t max_chains;  double gap_scale;
    uint32_t max_read_lookback_bases /* UINT32_MAX = none */, max_indel_bases;           /* used where the per-problem arrays are NULL */
} vgk_chain_scheme;
typedef struct vgk_chain_found { int32_t score; uint32_t item_begin, n_items, rec_begin, n_rec, n_rec_left; } vgk_chain_found;

int vgk_chain_items(vgk_ctx* ctx, const vgk_chain_scheme* scheme, uint32_t n_problems,
                    const uint64_t* anchor_off, const vgk_chain_anchor* anchors,
                    const uint64_t* cand_off, const vgk_chain_candidate* candidates,
                    const uint32_t* read_lookback /* [n], nullable */, const uint32_t* indel_limit /* [n], nullable */,
                    uint64_t* chain_off /* [n + 1] */, vgk_chain_found* chains, uint32_t* items, uint32_t* rec_right, uint32_t* rec_left,
                    int32_t* table_score /* nullable */, uint32_t* table_source /* nullable; UINT32_MAX = nowhere */);
/* out[0] = anchors of a problem whose table fits LDS (larger problems run over a slab in HBM), out[1] = the largest indel limit the penalty
 * tables take, out[2] = lanes per problem, out[3] = 0 (reserved).  Needs no context. */
int vgk_chain_items_limits(uint32_t out[4]);
/* Device time (ms) of the last vgk_chain_items call on this context: legality + grouping | DP | traceback */
int vgk_chain_items_last_ms(vgk_ctx* ctx, double ms[3]);

/* ---- anchors for chaining, from seeds and their gapless extensions ---------------------------------------------------------------------------
 * The step of MinimizerMapper::map_from_chains between vgk_gapless_extend and vgk_chain_items (src/minimizer_mapper_from_chains.cpp:1380-1596),
 * for thousands of (read, tree) problems per call: every seed's own anchor (to_anchor, :3978-4038); the seeds each extension contains
 * (extend_seed_group, src/minimizer_mapper.cpp:4881-5000 over for_each_read_interval, src/gbwt_extender.cpp:23-39); the full-length shortcut
 * (:1408-1464); the extensions in score order, each cut into read intervals around its mismatches (find_anchor_intervals, :480-706), every interval
 * welded from its first and last unused seed into one composite anchor (to_anchor, :4040-4081); sort_anchor_indexes.  No distance index and no zip
 * code is read.  The rule is the host shim's (vg_amd/host/extension_anchors.cpp), byte for byte.
 *
 * In: problem p's seeds are seeds[seed_off[p] .. seed_off[p + 1]) — node and diff exactly the vgk_seed the same seed gives vgk_gapless_extend,
 * stapled = Minimizer::pin_offset() (src/minimizer_mapper.hpp:596: a forward minimizer's first read base, a reverse one's last), length = k,
 * paths = the seed's haplotype flags; the seed's graph offset is stapled - diff.  Its extensions are extensions[ext_off[p] .. ext_off[p + 1]) as
 * vgk_gapless_extend wrote them WITHOUT VGK_GAPLESS_TRIM (the reference extends with trim == false here, src/minimizer_mapper.cpp:4863), with the
 * `nodes` and `mismatches` arrays they index; full_length[p] = vgk_gapless_result.full_length of the set.  match / mismatch: the plain scorer's
 * (a quality-adjusted context: VGK_EUNSUPPORTED).  VGK_ANCHORS_FROM_SEEDS in `flags` is do_gapless_extension == false: the anchors are the seed
 * anchors, sorted; ext_off and what follows it may then be NULL.
 *
 * Out: problem p's anchors are anchors[anchor_off[p] .. anchor_off[p + 1]) in sort_anchor_indexes' order — vgk_chain_items takes anchor_off and
 * anchors unchanged — and origins[] beside them: the first and last seed welded (numbers within the problem), n_seq = 1 or 2 seeds to paste into the
 * chain (extension_seed_sequences, :1575-1580), the seeds the anchor stands for in represented[rep_begin .. rep_begin + n_rep) (stapled order),
 * the extension it was cut from (number within the problem; UINT32_MAX in the seeds-only mode) and its read interval.  Problem p's stretch of
 * `represented` is rep_off[p] .. rep_off[p + 1].  status[p]: VGK_ANCHORS_FULL_LENGTH when the shortcut applies — the set is
 * full_length_extensions and some extension is full on both sides with at most default_max_extension_mismatches mismatches: no anchors then, and
 * the problem's stretch of `represented` lists those extensions' numbers instead, ascending.
 * Room: anchor_off, rep_off n_problems + 1; status n_problems; anchors / origins cap_anchors; represented cap_rep.  VGK_EOPS when either is too
 * small, with written[0] = the anchors and written[1] = the entries of `represented` there are (call with both 0 to size); never more than the
 * seeds, resp. the seeds plus the extensions, of the call.  A seed is used by one anchor at most.
 *
 * Ties the reference leaves open are fixed here [PARITY-UNPINNED]: seeds of one diagonal with equal stapled base by seed number (std::sort);
 * extensions of equal score by number (sort_permutation); anchors with equal read start and end in order of creation (std::sort).  Margins are
 * uint32 and wrap as the reference's size_t does when a reverse seed's minimizer begins before its interval.
 *
 * VGK_EINVAL: offsets that do not ascend from 0; a seed whose graph offset lies outside its node, of length 0, with is_reverse above 1, a reverse
 * seed stapled before base length - 1, stapled or length so large that a read position leaves int32; an extension whose path or mismatches leave
 * the arrays, whose read interval is empty or whose path is; mismatches not ascending inside the read interval; match or mismatch negative.
 * VGK_ETOOBIG: more than 2^32 - 16 seeds, extensions, path nodes or mismatches; or the problems' seeds x extensions summing above that (the bound on the
 * extensions' seed lists: split the call). */
typedef struct vgk_anchor_seed { uint32_t node; int32_t diff; uint32_t stapled; uint16_t length; uint16_t is_reverse; uint64_t paths; } vgk_anchor_seed;      /* 24 B */
typedef struct vgk_anchor_origin { uint32_t seed_first, seed_last, n_seq, rep_begin, n_rep, extension, read_begin, read_end; } vgk_anchor_origin;              /* 32 B */
#define VGK_ANCHORS_FROM_SEEDS  1u      /* in flags */
#define VGK_ANCHORS_FULL_LENGTH 1u      /* in status[p] */
int vgk_extension_anchors(vgk_ctx* ctx, const vgk_haplo* index, int32_t match, int32_t mismatch, uint32_t flags, uint32_t default_max_extension_mismatches,
                          uint32_t n_problems, const uint64_t* seed_off, const vgk_anchor_seed* seeds,
                          const uint64_t* ext_off, const vgk_extension* extensions, const uint32_t* full_length /* [n] */,
                          const uint32_t* nodes, size_t n_nodes, const uint32_t* mismatches, size_t n_mismatches,
                          uint64_t* anchor_off /* [n + 1] */, vgk_chain_anchor* anchors, vgk_anchor_origin* origins, size_t cap_anchors,
                          uint64_t* rep_off /* [n + 1] */, uint32_t* represented, size_t cap_rep, uint32_t* status /* [n] */, size_t written[2]);
/* out[0] = seeds of a problem whose used flags and sort keys fit LDS (larger problems run over a slab in HBM), out[1] = lanes per problem,
 * out[2] = extensions of a problem whose order fits LDS, out[3] = 0 (reserved).  Needs no context. */
int vgk_extension_anchors_limits(uint32_t out[4]);
/* Device time (ms) of the last vgk_extension_anchors call on this context: seed anchors + diagonal sort | the extensions' seed lists | the
 * order-dependent part, the sort and the write-out */
int vgk_extension_anchors_last_ms(vgk_ctx* ctx, double ms[3]);

/* ---- giraffe's alignments of a short read, composed on the device ----------------------------------------------------------------------------
 * What MinimizerMapper::map_from_extensions makes of an extension set once its tails are aligned (src/minimizer_mapper.cpp:934-1000): for a set
 * whose full_length is set, one alignment per leading extension that is full on both sides (extension_to_alignment :3905-3914 over
 * GaplessExtension::to_path, src/gbwt_extender.cpp:119-156); for any other set exactly two, the best and the second best of
 * find_optimal_tail_alignments (:5369-5622): min_tails, the two Pareto frontiers (:5263-5311, :5397-5419), the extensions in score order through
 * process_until_threshold_e (src/minimizer_mapper.hpp:1580-1659) with the score-estimate skip (:5453-5479), the totals, the winner and the runner-up
 * that differs from it at both end nodes (:5545-5590), the tails' Paths as get_best_alignment_against_any_tree returns them (:5626-5743; a left
 * tail flipped as reverse_complement_path does) and the concatenation by add_to_path (:5318-5367) — no simplify.  No distance index and no zip code
 * is read.  The rule is stated serially in vg_amd/csrc/read_alignments_device.hpp (ra_read_one), which the kernels call.
 *
 * In: read r is reads[read_off[r] .. read_off[r + 1]) as the caller holds it (a base that is not one of ACGT never matches); results[r] its
 * vgk_gapless_result, with the `extensions`, `nodes` and `mismatches` arrays of the vgk_gapless_extend call; `tails` and `ops` exactly as
 * vgk_tail_stage_aligned returned them for those extensions (in any order).  An open end without a tail entry, and a tail with n_ops 0, is the soft
 * clip.  Scores are the context's: match = matrix[0], mismatch = -matrix[1], gap open / extend, full-length bonus; a quality-adjusted context:
 * VGK_EUNSUPPORTED.
 *
 * Out: read r's alignments are alignments[aln_off[r] .. aln_off[r + 1]): VGK_READ_ALN_DIRECT ones in set order, or BEST then SECOND (either may be
 * empty: score 0, no mappings, extension = UINT32_MAX).  A header begins with the fields of vgk_chain_result, so that mappings and edit runs are
 * laid out as vgk_chain_stitch's: per mapping {oriented node, offset, edit_begin, n_edits}, ranks = index + 1; per edit length << 2 | VGK_WFA_*.
 * Every mismatch is a one-base edit of its own, match runs lie between them, soft clips are insertions; inserted and substituted bases are the read's
 * own.  identity = identity_num / identity_den (0 when identity_den is 0): identity(path) for BEST / SECOND, (len - mismatches) / len for DIRECT.
 * A read whose input is malformed, or whose gapless result failed, has ONE header with that status and nothing else.
 * Room: aln_off n + 1; VGK_EOPS when cap_alignments, cap_mappings or cap_edits is too small, with written[0..2] = the alignments, mappings and
 * edit runs there are (call with all three 0 to size); nothing is written past a capacity.
 *
 * [PARITY-UNPINNED] the reference shuffles the extensions that tie for the top score with the read's generator (sort_shuffling_ties,
 * src/utility.hpp:771-794), whose state depends on everything drawn earlier in the read's life: here ties stay in extension order.  Node ids are
 * (oriented node >> 1) + 1, so that 0 stays "none yet" as at :5545-5556.  Consecutive ops of a tail on one oriented node are one mapping, until
 * the node's bases are spent and an M or D op follows: that is a second visit (a self-loop), a mapping of its own at offset 0.
 *
 * Per read VGK_EINVAL (the read's one header; the call goes on): ext_begin + n_ext beyond the extensions; a path or mismatch list beyond its array,
 * an empty path, a node outside the index, offset outside the first node, a read interval that is empty or leaves the read, a path that does not
 * hold the interval's bases exactly; mismatches outside [read_begin, read_end) or not ascending; left_full / right_full that disagree with the
 * interval; full_length set on a set whose first extension is not full; a tail on a closed end, a second tail for one end, read_begin / read_end
 * that are not the open end's, ops beyond their array, an op of length 0, of an unknown kind or on a node outside the index, ops that spend more
 * read bases than the tail has or more bases of a node than it has.  For the call: VGK_EINVAL offsets that do not ascend from 0, a tail whose `ext`
 * is beyond the extensions, unknown flags, window_length 0; VGK_ETOOBIG more than 2^32 - 16 of anything, or a bound on the output beyond that. */
typedef struct vgk_read_alignments_policy {
    uint32_t extension_score_threshold;   /* MinimizerMapper's field of that name (default 1) */
    uint32_t max_local_extensions;        /* 0xffffffff: no limit */
    uint32_t window_length;               /* k + w - 1, or k with syncmers */
    uint32_t flags;                       /* 0 */
} vgk_read_alignments_policy;
enum { VGK_READ_ALN_DIRECT = 0, VGK_READ_ALN_BEST = 1, VGK_READ_ALN_SECOND = 2 };
typedef struct vgk_read_alignment {      /* 56 B; the first 32 are a vgk_chain_result */
    int32_t  status;
    uint32_t mapping_begin, n_mappings;
    uint32_t edit_begin, n_edits;
    uint32_t from_length, to_length;
    uint32_t read;                        /* the read it belongs to */
    uint32_t kind;                        /* VGK_READ_ALN_* */
    uint32_t extension;                   /* index into `extensions`; UINT32_MAX: none (an empty BEST / SECOND) */
    int32_t  score;
    uint32_t identity_num, identity_den;
    uint32_t reserved;
} vgk_read_alignment;
int vgk_read_alignments(vgk_ctx* ctx, const vgk_haplo* index, const vgk_read_alignments_policy* policy,
                        const char* reads, const uint64_t* read_off, uint32_t n, const vgk_gapless_result* results,
                        const vgk_extension* extensions, size_t n_extensions, const uint32_t* nodes, size_t n_nodes, const uint32_t* mismatches, size_t n_mismatches,
                        const vgk_tail_alignment* tails, size_t n_tails, const vgk_op* ops, size_t n_ops,
                        uint64_t* aln_off /* [n + 1] */, vgk_read_alignment* alignments, size_t cap_alignments,
                        vgk_chain_mapping* mappings, size_t cap_mappings, uint32_t* edits, size_t cap_edits, size_t written[3]);
/* The resident form: vgk_tail_stage_aligned (vgk.h) followed by the same kernels over what lies in HBM — the sets the last vgk_gapless_extend(_seeded)
 * call on this context left there, with their masked reads, and the tails' winning alignments and ops, which are made and consumed on the device: only
 * ext_total, read_score (as vgk_tail_stage's) and the composed alignments cross PCIe.  The alignments are those vgk_read_alignments makes of the same
 * call's downloaded sets and tails, byte for byte.  Outputs, capacities, VGK_EOPS and written[0..2] as vgk_read_alignments' (ext_total and read_score are
 * complete on VGK_EOPS too: call again with the room named, after extending again); a VGK_GAPLESS_DEFER call's copies are finished when this call
 * returns, as by the other two tail-stage entry points.  The sets are the engine's own: nothing is validated per read; a read whose extension failed
 * has one header with that status. */
int vgk_tail_stage_composed(vgk_ctx* ctx, const vgk_haplo* index, uint32_t ops_per_problem, const vgk_read_alignments_policy* policy,
                            int32_t* ext_total, size_t ext_cap, int32_t* read_score,
                            uint64_t* aln_off /* [reads + 1] */, vgk_read_alignment* alignments, size_t cap_alignments,
                            vgk_chain_mapping* mappings, size_t cap_mappings, uint32_t* edits, size_t cap_edits, size_t written[3], uint64_t stats[4]);
/* out[0] = extensions of a set whose order and frontiers the selection keeps in LDS (a lane per read; larger sets run over a slab in HBM),
 * out[1] = lanes per read in the selection, out[2] = lanes per read in count and emit, out[3] = 0 (reserved).  Needs no context. */
int vgk_read_alignments_limits(uint32_t out[4]);
/* Device time (ms) of the last vgk_read_alignments call on this context: selection | count + prefix sums | emit */
int vgk_read_alignments_last_ms(vgk_ctx* ctx, double ms[3]);

/* ---- a read's mapping quality on the device: the alignments' scores and the explored-minimizer cap --------------------------------------------
 * What both mapping routes close with (MinimizerMapper::map, src/minimizer_mapper.cpp:1143-1188; map_from_chains,
 * src/minimizer_mapper_from_chains.cpp:957-1057): the mapping quality of the alignments' scores (MappingQualityCalculator's exact form), capped by
 * faster_cap over the explored minimizers (:2946-3260, the Phred-scaled probability that sequencing errors created all of them), the escape bonus,
 * round, clamp to 0 .. 60.  The rule is stated serially in vg_amd/csrc/read_mapq_device.hpp (mq_region_one, mq_read_one), which the kernels call.
 *
 * vgk_minimizer_regions: per minimizer of a list as vgk_minimizer_list / vgk_minimizer_find_seeds answer it (offset order per read; any list: no
 * index is needed, hash = Thomas Wang's mix of the key) its agglomeration {start, length} in read bases: from the start of the first window the
 * instance wins to the end of the last (window s = k-mers [s, s + w) = bases [s, s + w + k - 1); its minimizer is the leftmost smallest canonical
 * hash among its valid k-mers; src/minimizer_mapper.hpp:565-600).  Only the list is read: an instance's windows follow from its two neighbours.
 * VGK_EINVAL for the call: k or w outside what the index takes, offsets that do not ascend from 0, a minimizer that does not fit its read or whose
 * read has no complete window, a list out of offset order; VGK_ETOOBIG beyond 2^32 - 16 minimizers.
 *
 * vgk_read_mapq: per read r
 *   scores[score_off[r] .. score_off[r + 1])  the alignments' scores in the reference's `scores` order (the log-sum runs backwards over it), with
 *   multiplicity (nullable; as long as scores) and unmapped[r] (nullable; non-zero: the first alignment has no mappings, mapping quality 0);
 *   minimizers[minimizer_off[r] .. minimizer_off[r + 1]) with their regions and explored (one byte each, non-zero: the minimizer was explored);
 *   read_off for the length; quality (nullable: the cap is +infinity, as faster_cap returns) holds read r's Phred bytes at read_off[r].
 * A minimizer's forward_offset is its offset (the k-mer's first base), its length is the scheme's k — or, under VGK_READ_MAPQ_OWN_LENGTH, its own
 * `reserved` field (the lists of the reference's unit tests hold minimizers of several lengths).
 * Out, per read: mapq = clamp(round(min(bonus * explored_cap, uncapped)), 0, 60) with bonus = 2 where uncapped is INT32_MAX, else 1; uncapped = the
 * scores' mapping quality after the reference's (int32_t) truncation (INT32_MAX: infinite; 0 for an unmapped read); explored_cap = the cap before the
 * bonus (+infinity without qualities or under VGK_READ_MAPQ_NO_EXPLORED_CAP; -0.0 when nothing was explored, as in the reference).
 * status VGK_EINVAL, with mapq 0, for a read on which the reference stops — a mapped read without scores, an explored minimizer of length 0,
 * "minimizers seem impossible to disrupt" (a column's probability underflows to 0), "not sorted / stacked properly" (unreachable once the
 * explored minimizers are sorted, kept as the reference keeps it) — or whose explored minimizer is longer than the 32 events the probability table holds
 * or has an agglomeration that begins behind the read's last base (the reference would read qualities that are not there).
 * For the call: VGK_EINVAL offsets that do not ascend from 0, unknown flags, a log_base or score_scale that is not finite and positive;
 * VGK_ETOOBIG beyond 2^32 - 16 of anything, or 2^24 minimizers in one read.  Ties of (agglomeration end, start) among explored minimizers keep list order
 * (the reference leaves them to std::sort; agglomerations as vgk_minimizer_regions makes them never tie). */
typedef struct vgk_minimizer_region { uint32_t start, length; } vgk_minimizer_region;
enum { VGK_READ_MAPQ_FIRST = 1,            /* compute_first_mapping_quality: the chain route's form (default: compute_max_mapping_quality) */
       VGK_READ_MAPQ_NO_EXPLORED_CAP = 2,  /* use_explored_cap == false */
       VGK_READ_MAPQ_OWN_LENGTH = 4 };     /* a minimizer's length is its `reserved` field */
typedef struct vgk_read_mapq_scheme {
    double   log_base;                    /* the scorer's, as MappingQualityCalculator takes it */
    double   score_scale;                 /* mapq_score_scale (1.0: off) */
    uint32_t score_window;                /* mapq_score_window (0: off) */
    uint32_t k;
    uint32_t flags;                       /* VGK_READ_MAPQ_* */
    uint32_t reserved;
} vgk_read_mapq_scheme;
typedef struct vgk_read_mapq_result { int32_t mapq; int32_t status; double uncapped; double explored_cap; } vgk_read_mapq_result;      /* 24 B */
int vgk_minimizer_regions(vgk_ctx* ctx, uint32_t k, uint32_t w, const uint64_t* read_off, uint32_t n, const uint64_t* minimizer_off,
                          const vgk_read_minimizer* minimizers, vgk_minimizer_region* regions);
int vgk_read_mapq(vgk_ctx* ctx, const vgk_read_mapq_scheme* scheme, uint32_t n, const uint64_t* score_off, const int32_t* scores, const double* multiplicity,
                  const uint8_t* unmapped, const uint64_t* minimizer_off, const vgk_read_minimizer* minimizers, const vgk_minimizer_region* regions,
                  const uint8_t* explored, const uint64_t* read_off, const uint8_t* quality, vgk_read_mapq_result* out /* [n] */);
/* out[0] = explored minimizers of a read whose order and c[] table the sweep keeps in LDS (a lane per read; reads with more run in a second launch
 * over a slab in HBM), out[1] = lanes per read in the sweep, out[2] = lanes per minimizer in vgk_minimizer_regions, out[3] = 0 (reserved) */
int vgk_read_mapq_limits(uint32_t out[4]);
/* Device time (ms) of the last vgk_minimizer_regions | vgk_read_mapq call on this context */
int vgk_read_mapq_last_ms(vgk_ctx* ctx, double ms[2]);
/* Reads of the last vgk_read_mapq call by where they ran: swept in LDS | swept over the slab | not swept (refused by the checks) */
int vgk_read_mapq_last_launches(vgk_ctx* ctx, uint64_t reads[3]);

/* ---- a pair's mapping qualities on the device: pair scores, their order, the caps both mates share ---------------------------------------------
 * What MinimizerMapper::map_paired closes with (src/minimizer_mapper.cpp:2476-2765; score_alignment_pair :6017-6028): the score of every
 * candidate pairing, the score order with the max_multimaps cut, the multiplicities of rescued pairs, the pair's uncapped quality, the
 * fragment-cluster cap, the two mates' explored caps summed, the unpaired cap, the halving for unreachable mates, and
 * max(min(capped, 120) / 2, 0) truncated to the integer both mates carry.  Arithmetic on small per-pair lists: no distance index, no zip code, no
 * graph.  The rule is stated serially in vg_amd/csrc/pair_mapq_device.hpp (pm_candidate_score, pm_pair_one), which the kernels call.
 *
 * Pair p is reads 2 p and 2 p + 1.  Per pair:
 *   candidates[cand_off[p] .. cand_off[p + 1])  the entries of the reference's paired_alignments in creation order: the mates' alignment scores;
 *     distance = what distance_between returned (INT64_MAX: unreachable; an UNPAIRED candidate counts as INT64_MAX whatever it holds); aln[r] = the
 *     number of mate r's alignment among the pair's alignments of that mate (equal number = the same alignment; only the score groups read it);
 *     better_cluster_count; type = the reference's PairType; aligned: bit r is set when mate r's alignment has mappings.
 *   counts[p]  unpaired_count and rescued_count per mate.
 *   unpaired_scores[unpaired_off[2 p + r] .. unpaired_off[2 p + r + 1])  mate r's unpaired alignments' scores (either pointer NULL: empty
 *     everywhere); read only when the winner's type is UNPAIRED.
 *   explored caps: given_cap[2 n] (for instance explored_cap of an earlier vgk_read_mapq) — or, when given_cap is NULL, vgk_read_mapq's minimizer
 *     arguments for the 2 n reads: the call then runs that entry's sweep for both mates on the device and the caps stay in HBM for the pair kernels.
 *     VGK_PAIR_MAPQ_NO_EXPLORED_CAP, or given_cap and quality both NULL: +infinity.
 * The rule, in order.  (1) A candidate's pair score: for a rescued type whose rescued mate is not aligned, (double) the mapped mate's score
 * (:2386-2391); otherwise score_alignment_pair: dev = distance - mean, ll = (-dev * dev / (2.0 * sd * sd)) / log_base,
 * max(score0 + score1 + ll, min(score0, score1)), the integer sum first.  (2) Order: pair score descending (process_until_threshold_a with
 * threshold 0, src/minimizer_mapper.hpp:1580-1659); equal scores stay in candidate order (the reference shuffles them with the read's generator:
 * not pinned here); the first min(C, max_multimaps) are the mappings, all C scores in this order feed the quality.  (3) Multiplicities
 * (:2660-2685): est[r] = unpaired_count[r] > 0 ? unpaired_count[r] / min(rescued_count[r], max_rescue_attempts) : 1.0; 1 for PAIRED and UNPAIRED,
 * est[0] for RESCUED_FROM_FIRST, est[1] for RESCUED_FROM_SECOND; used only when no candidate is PAIRED.  (4) uncapped = 0 when the first ordered
 * score is 0, else compute_max_mapping_quality (exact form, int32 truncation) over log_base * score.  (5) fragment_cluster_cap =
 * -10 log10(1 - 1 / n) for the winner's better_cluster_count n > 1, else +infinity.  (6) Score groups (:2524-2546, :2704; annotation only, never
 * applied): when the pair has a PAIRED candidate, group r = the winner's score, then — if the winner is PAIRED — the scores of the other PAIRED
 * candidates with the winner's aln[r], in candidate order; score_group[r] = compute_max_mapping_quality of it (INT32_MAX for an empty group).
 * (7) Per mate r (:2727-2765): bonus = 2 when uncapped is INT32_MAX, else 1; cap = min(fragment_cluster_cap, (explored_cap[0] + explored_cap[1]) *
 * bonus), for an UNPAIRED winner also min with compute_max_mapping_quality(unpaired_scores[r]); capped = min(cap, uncapped), halved when the
 * winner's distance is INT64_MAX; mapq[r] = (int32_t) max(min(capped, 120.0) / 2.0, 0.0), and 0 when the winner's mate r is not aligned.
 * (8) A pair without candidates: both qualities 0, n_chosen 0, fragment_cluster_cap and score_group +infinity / INT32_MAX as above.
 * Out, per pair: the 80-byte result (applied_cap[r] = the cap of step 7); per candidate pair_score (candidate order; a candidate's own, whatever
 * becomes of its pair; 0 for a type above 3) and order (the candidate numbers within the pair in score order, laid out on cand_off; candidate
 * order for a refused pair).
 * Per pair VGK_EINVAL with everything else 0 (the call goes on): a type above 3; a rescued-type candidate when min(rescued_count,
 * max_rescue_attempts) of its side is 0; an unaligned rescued mate with a finite distance; either mate stopped by the sweep (vgk_read_mapq's
 * per-read refusals, less the one about scores).  For the call: VGK_EINVAL offsets that do not ascend from 0, unknown flags, log_base or
 * fragment_sd not finite and positive, fragment_mean not finite; VGK_ETOOBIG beyond 2^32 - 16 of anything (2 n reads included).
 * Out of scope: identify_supplementary_alignments; the max_rescue_attempts == 0 early return with quality 1 (:2238-2287); deriving
 * better_cluster_count (:1653-1690) and distance_between, which are inputs; the proper-pair annotation. */
enum { VGK_PAIR_PAIRED = 0, VGK_PAIR_UNPAIRED = 1, VGK_PAIR_RESCUED_FROM_FIRST = 2, VGK_PAIR_RESCUED_FROM_SECOND = 3 };
enum { VGK_PAIR_MAPQ_NO_EXPLORED_CAP = 1 };
typedef struct vgk_pair_candidate {
    int32_t  score[2];
    int64_t  distance;
    uint32_t aln[2];
    uint32_t better_cluster_count;
    uint8_t  type;                        /* VGK_PAIR_* */
    uint8_t  aligned;                     /* bit r: mate r's alignment has mappings */
    uint16_t reserved;
} vgk_pair_candidate;                     /* 32 B */
typedef struct vgk_pair_counts { uint32_t unpaired_count[2], rescued_count[2]; } vgk_pair_counts;
typedef struct vgk_pair_mapq_scheme {
    double   log_base;                    /* the scorer's */
    double   fragment_mean, fragment_sd;  /* fragment_length_distr */
    uint32_t max_multimaps, max_rescue_attempts;
    uint32_t k;                           /* the minimizers' length, for the sweep */
    uint32_t flags;                       /* VGK_PAIR_MAPQ_* */
} vgk_pair_mapq_scheme;
typedef struct vgk_pair_mapq_result {
    int32_t  mapq[2];
    int32_t  status;
    uint32_t n_chosen;                    /* min(candidates, max_multimaps) */
    double   uncapped, fragment_cluster_cap, explored_cap[2], score_group[2], applied_cap[2];
} vgk_pair_mapq_result;                   /* 80 B */
int vgk_pair_mapq(vgk_ctx* ctx, const vgk_pair_mapq_scheme* scheme, uint32_t n /* pairs */, const uint64_t* cand_off, const vgk_pair_candidate* candidates,
                  const vgk_pair_counts* counts, const uint64_t* unpaired_off /* [2 n + 1] */, const int32_t* unpaired_scores, const double* given_cap /* [2 n] */,
                  const uint64_t* minimizer_off, const vgk_read_minimizer* minimizers, const vgk_minimizer_region* regions, const uint8_t* explored,
                  const uint64_t* read_off, const uint8_t* quality, vgk_pair_mapq_result* out /* [n] */, double* pair_score, uint32_t* order);
/* out[0] = candidates of a pair whose order and ordered scores the pair kernel keeps in LDS (a lane per pair; pairs with more run in a second launch
 * over a slab in HBM), out[1] = lanes per pair, out[2] = lanes per candidate in the score kernel, out[3] = 0 (reserved) */
int vgk_pair_mapq_limits(uint32_t out[4]);
/* Device time (ms) of the last vgk_pair_mapq call on this context: the mates' sweep (0 with given caps) | the score and pair kernels */
int vgk_pair_mapq_last_ms(vgk_ctx* ctx, double ms[2]);
/* Pairs of the last vgk_pair_mapq call by where they ran: in LDS | over the slab | refused by the call's own checks (a stopped mate is found on
 * the device and counts where its pair ran) */
int vgk_pair_mapq_last_launches(vgk_ctx* ctx, uint64_t pairs[3]);
/* Kernels the last vgk_pair_mapq call launched, counted where they are launched: the mates' sweep (0 with given caps; 2 when some read went over
 * the slab) | the score kernel and the pair kernels (a launch list that is empty launches nothing) */
int vgk_pair_mapq_last_kernel_launches(vgk_ctx* ctx, uint32_t launches[2]);

/* ---- a short read's funnel on the device: which clusters are extended, which sets are aligned, which alignments win ------------------------------
 * The three decisions MinimizerMapper::map_from_extensions makes between the stages above (src/minimizer_mapper.cpp:650-1128), for the default
 * find_supplementaries == false, over flat arrays and with the clusters GIVEN (as vgk_chain_items takes its transitions): no distance index is
 * read.  The rule is stated serially in vg_amd/csrc/read_funnel_device.hpp (rf_walk and the rf_*_one around it), which the kernels call; the host
 * shim (vg_amd/host/read_funnel.cpp: vgh_funnel_*) states it in the reference's loop shape and is the checker.
 *
 * The walk all three share is process_until_threshold_e (src/minimizer_mapper.hpp:1580-1659) with the escape always false: std::stable_sort by
 * a comparator; the w >= 2 items tied at the top shuffled; better_or_equal; cutoff = best - threshold; an item fails the threshold when
 * threshold != 0 && score <= cutoff, unless fewer than `min` items were accepted; any other item is accepted while fewer than `max` were; only
 * items the step itself accepts count towards min and max.
 *
 * vgk_funnel_clusters.  Read r: its length from read_off; its minimizers minimizers[minimizer_off[r] ..) (the k-mer covers offset .. offset + length,
 * length = policy->k, or the `reserved` field with VGK_FUNNEL_OWN_LENGTH); minimizer_score[] one double per minimizer as score_minimizers makes them
 * (no logarithm is computed here); its clusters cluster_off[r] .. cluster_off[r + 1]; cluster c's seeds sources[cluster_seed_off[c] ..
 * cluster_seed_off[c + 1]), each the number WITHIN THE READ of the minimizer the seed came from (Seed::source).  Per cluster (score_cluster, :4738-4770):
 * score = the scores of the DISTINCT minimizers present, added in ascending minimizer number; covered = the read bases under some present k-mer (a
 * union); coverage = (double) covered / (double) length; then the walk of :711-832 by coverage descending, then score descending, with
 * cluster_coverage_threshold, min_extensions, max_extensions and, inside it, the score filter of :746-747 against the padded cutoff of :685-688
 * (strict <): verdict, rank (position in the walk's order) and better_or_equal (for every item, not only those processed).  Per read:
 * kept[kept_off[r] .. kept_off[r + 1]) = the clusters extended, in the order extended (the order of cluster_extensions, so the numbering of the
 * sets below), as indices into the call's flat cluster arrays.
 *
 * vgk_funnel_extension_sets.  Read r's sets are results[set_off[r] .. set_off[r + 1]), one vgk_gapless_result per kept cluster in kept order (the
 * caller ran vgk_gapless_extend with one problem per kept cluster), over `extensions`; set_off must equal kept_off.  Gap open and gap extend are
 * the context's; a quality-adjusted context: VGK_EUNSUPPORTED.  Per set: estimate = score_extension_group (:5022-5243; a full-length set: its first
 * extension's score; an empty set: 0; a failed gapless result: 0 and verdict FAILED, never aligned, never counted); the walk of :887-1063 by
 * estimate descending with extension_set_score_threshold, min_extension_sets, max_alignments: ALIGN, FAIL_SCORE (the threshold), FAIL_MIN_SCORE
 * (estimate < extension_set_min_score when processed: skipped, counts towards neither min nor max) or FAIL_MAX_ALIGNMENTS; rank, better_or_equal.
 * Per read: aligned[aligned_off[r] ..) = the sets aligned, in walk order, as indices into `results`; explored[] one byte per minimizer, set when
 * the minimizer has a seed in a cluster whose set got ALIGN (:1036-1043) — what vgk_read_mapq takes.
 *
 * vgk_funnel_winners.  Read r's aligned sets are entries aligned_off[r] .. aligned_off[r + 1] of the aligned list; entry j's alignments, as
 * vgk_read_alignments ordered them, are aln_score / aln_mappings[aln_off[j] .. aln_off[j + 1]) (score, n_mappings).  Per set the loop of :1025:
 * alignments are kept while the score is non-zero and at least 0.8 of the set's FIRST alignment's score (compared in double), stopping at the
 * first that fails.  Nothing kept: one unaligned entry, score 0, pick (0xffffffff, 0xffffffff).  Then the walk of :1095-1128 by score descending,
 * threshold 0, min 1, max max_multimaps (0: VGK_EINVAL).  scores[score_off[r] ..) = every kept score in walk order, those beyond max_multimaps
 * included: vgk_read_mapq's `scores`.  reported[] lies on score_off as well: the (aligned-list entry, alignment within it) pair of every score; the
 * first n_reported[r] = min(count, max_multimaps) of them are the mappings.  unmapped[r] = the first one has no mappings (:1146).
 *
 * rng_state (all three calls; uint32 per read, in/out, nullable): the state of the read's std::minstd_rand; 0 = not made yet; made at the first
 * draw from the read's bytes (`reads`, required with rng_state, otherwise nullable and unread) exactly as find_seeds' sort makes it
 * (seed = seed * 13 + byte; state = seed mod (2^31 - 1), 1 for 0).  A run of w >= 2 items tied at the top of a walk costs w - 1 draws,
 * x[rng() % (i + 1)] <-> x[i] for i = 1 .. w - 1 (deterministic_shuffle, src/utility.hpp:721-728); everything else stays in std::stable_sort order.
 * With NULL nothing is shuffled and ties stay in index order, as vgk_read_alignments leaves them.  Carried through vgk_minimizer_find_seeds' sort
 * (whose state the caller replays: that entry does not export it), the cluster walk, the set walk and the winner walk, the state models every draw of
 * a single-end read's life but those inside find_optimal_tail_alignments (:984), which vgk_read_alignments does not make. [PARITY-UNPINNED: the
 * reference holds no test of these draws; std::sort freedoms the reference leaves open do not arise here: every order is std::stable_sort's.]
 *
 * Sizing: kept_cap / aligned_cap / score_cap with written[0] = what the call has; VGK_EOPS when the capacity is short — the offsets, the per-item
 * outputs and written[] are complete even then (rng_state is advanced by every call that gets that far: size with a copy of it).
 * Per read, status[r] = VGK_EINVAL with the read's outputs zeroed and nothing kept (the call goes on): a source beyond the read's minimizers, a
 * k-mer that leaves the read, a read of length 0 that has clusters, a minimizer score that is not finite; for the sets also a kept cluster or an
 * extension range beyond the arrays, an extension that leaves the read, is empty, or starts before its predecessor.  For the call VGK_EINVAL:
 * offsets that do not ascend from 0, a threshold that is not finite, unknown flags, set_off that disagrees with kept_off, rng_state without reads;
 * VGK_ETOOBIG beyond 2^32 - 16 of anything. */
enum { VGK_FUNNEL_OWN_LENGTH = 1 };       /* policy flags: a minimizer's length is its `reserved` field, as VGK_READ_MAPQ_OWN_LENGTH */
enum { VGK_FUNNEL_UNDECIDED = 0,          /* (a refused read's items) */
       VGK_FUNNEL_EXTEND = 1, VGK_FUNNEL_FAIL_COVERAGE = 2, VGK_FUNNEL_FAIL_SCORE = 3, VGK_FUNNEL_FAIL_MAX_EXTENSIONS = 4 };
enum { VGK_FUNNEL_SET_ALIGN = 1, VGK_FUNNEL_SET_FAIL_SCORE = 2, VGK_FUNNEL_SET_FAIL_MIN_SCORE = 3, VGK_FUNNEL_SET_FAIL_MAX_ALIGNMENTS = 4, VGK_FUNNEL_SET_FAILED = 5 };
typedef struct vgk_funnel_policy {        /* MinimizerMapper's fields of the same names; giraffe's defaults in brackets */
    double   cluster_score_threshold;     /* [50] */
    double   pad_cluster_score_threshold; /* [20] */
    double   cluster_coverage_threshold;  /* [0.3] */
    double   extension_set_score_threshold;   /* [20] */
    int32_t  extension_set_min_score;     /* [20] */
    uint32_t min_extensions, max_extensions;  /* [2] [800] */
    uint32_t min_extension_sets, max_alignments;  /* [2] [8] */
    uint32_t max_multimaps;               /* [1] */
    uint32_t k;
    uint32_t flags;                       /* VGK_FUNNEL_* */
} vgk_funnel_policy;                      /* 64 B */
typedef struct vgk_funnel_cluster { double score, coverage; uint32_t covered, rank, better_or_equal, verdict; } vgk_funnel_cluster;      /* 32 B */
typedef struct vgk_funnel_set { int32_t estimate; uint32_t rank, better_or_equal, verdict; } vgk_funnel_set;                           /* 16 B */
typedef struct vgk_funnel_pick { uint32_t set, alignment; } vgk_funnel_pick;
int vgk_funnel_clusters(vgk_ctx* ctx, const vgk_funnel_policy* policy, uint32_t n, const char* reads, const uint64_t* read_off,
                        const uint64_t* minimizer_off, const vgk_read_minimizer* minimizers, const double* minimizer_score,
                        const uint64_t* cluster_off, const uint64_t* cluster_seed_off, const uint32_t* sources, uint32_t* rng_state,
                        vgk_funnel_cluster* clusters, int32_t* status /* [n] */, uint64_t* kept_off /* [n + 1] */, uint32_t* kept, size_t kept_cap, size_t written[1]);
int vgk_funnel_extension_sets(vgk_ctx* ctx, const vgk_funnel_policy* policy, uint32_t n, const char* reads, const uint64_t* read_off,
                              const uint64_t* set_off, const vgk_gapless_result* results, const vgk_extension* extensions, size_t n_extensions,
                              const uint64_t* kept_off, const uint32_t* kept, const uint64_t* cluster_seed_off, size_t n_clusters, const uint32_t* sources,
                              const uint64_t* minimizer_off, uint32_t* rng_state,
                              vgk_funnel_set* sets, int32_t* status /* [n] */, uint64_t* aligned_off /* [n + 1] */, uint32_t* aligned, size_t aligned_cap,
                              uint8_t* explored, size_t written[1]);
int vgk_funnel_winners(vgk_ctx* ctx, const vgk_funnel_policy* policy, uint32_t n, const char* reads, const uint64_t* read_off,
                       const uint64_t* aligned_off, const uint64_t* aln_off, const int32_t* aln_score, const uint32_t* aln_mappings, uint32_t* rng_state,
                       uint64_t* score_off /* [n + 1] */, int32_t* scores, vgk_funnel_pick* reported, size_t score_cap,
                       uint32_t* n_reported /* [n] */, uint8_t* unmapped /* [n] */, size_t written[1]);
/* What a lane keeps in LDS; items beyond run in a second launch over a slab in HBM.  out[0] = minimizers of a read (a cluster's present bits),
 * out[1] = bases of a read (a cluster's covered bitmap), out[2] = items of a walk (a read's clusters, sets or kept alignments), out[3] = extensions
 * of a set (the estimate's chain table).  A lane per cluster or set for the scoring, a lane per read for the walks. */
int vgk_funnel_limits(uint32_t out[4]);
/* Device time (ms) of the last vgk_funnel_clusters | vgk_funnel_extension_sets | vgk_funnel_winners call on this context */
int vgk_funnel_last_ms(vgk_ctx* ctx, double ms[3]);
/* Reads of the last vgk_funnel_* call by where they ran: every item of theirs in LDS | the walk or some cluster or set of theirs over the slab |
 * refused by the checks */
int vgk_funnel_last_launches(vgk_ctx* ctx, uint64_t reads[3]);

/* ---- a chain's links on the device: what find_chain_alignment's walk decides to align, and how ---------------------------------------------------
 * The first half of MinimizerMapper::find_chain_alignment (src/minimizer_mapper_from_chains.cpp:2576-3292, its decisions only): the step between
 * vgk_chain_items, which answers with chains of anchor numbers, and the chain stage (vg_amd/host/chain_stage.hpp), which takes a finished link
 * table and the kept anchors.  No distance index is read: the distances the walk asks for are GIVEN, as vgk_chain_items is given its transitions.
 * The rule is stated serially in vg_amd/csrc/chain_links_device.hpp (cl_walk_one and cl_slot), which the kernels call; the host shim
 * (vg_amd/host/chain_links.cpp: vgh_chain_links) states it in the reference's loop shape and is the checker.  No reference unit test names
 * find_chain_alignment [PARITY-UNPINNED]: the rule is held to a second statement in tests/test_chain_links.py.
 *
 * In.  Reads as `reads` / read_off[n_reads + 1].  Anchor sets exactly as vgk_chain_items takes and leaves them: set s's anchors are
 * anchors[anchor_off[s] .. anchor_off[s + 1]) (read_start and length are read), sites[] one per anchor beside them — graph_start =
 * (start_node, start_offset), graph_end = (end_node, end_offset), oriented nodes, end_offset past the end within end_node and so at least 1,
 * bit 0 of flags = Anchor::is_skippable() — and `items` (n_items entries) the flat item array of vgk_chain_items.  Chain p is
 * {read, anchor_set, item_begin, n_items}: items[item_begin .. item_begin + n_items), anchor numbers within the set, left to right; several chains
 * may share a read or a set.  Set s's distances are dist[dist_off[s] .. dist_off[s + 1]) as vgk_chain_candidate {from, to, graph_distance}:
 * graph_distance is what algorithms::get_graph_distance(from, to) answers — end of `from` to start of `to`, NOT the hint distance — strictly
 * ascending by (from, to); a pair that is absent (or given as UINT32_MAX) is unreachable, SIZE_MAX in the walk.  The walk asks for (here, next) and,
 * inside the skip loop, for consecutive items (skip_to, skip_to + 1).
 *
 * The walk (arithmetic in uint64, the reference's size_t): left tail of here.read_start bases (:2611): at most max_tail_length -> WFA, PREFIX, to =
 * graph_start(here); at most max_tail_dp_length -> DP; longer -> SOFTCLIP (an insertion without a position, score 0, :2667-2680).  Next anchor
 * (:2758-2778): items with next.read_start < here.read_end are passed over; none left: the chain ends at here.  Skip past repetitive anchors
 * (:2786-2863) in the reference's loop shape: strict < against max_skipped_bases, strict > against min_indel_avoid_bases, never past the chain's
 * last item, += skip_to->length() on both distances.  The link here -> next (:2909-3001, :3044-3051): link_length = next.read_start -
 * here.read_end, graph_dist as given; both 0 -> EMPTY; else 0 < link_length <= max_chain_connection && graph_dist * link_length <= max_dp_cells ->
 * WFA, CONNECT, from = graph_end(here) with its offset - 1, to = graph_start(next); else link_length > max_middle_dp_length || graph_dist *
 * link_length > max_dp_cells -> REFUSED: no link is written, the chain ends at here (kept), VGK_CHAIN_LINKS_CUT is set and the right tail starts at
 * here.read_end; else -> DP (length 0 allowed: a pure deletion).  Right tail (:3152-3283): read length - here.read_end bases, SUFFIX, from =
 * graph_end(here) with its offset - 1, classed as the left one.  Kept anchors: `here` at every step.  anchor_score = the sum over them of match *
 * length, + full_length_bonus for one that starts at read base 0 and for one that ends at the read's end (to_wfa_alignment, :4083-4104).  Plain
 * scoring only: a quality-adjusted context answers VGK_EUNSUPPORTED.
 * THE WRAP: graph_dist * link_length, total_graph_distance + cur_graph_distance and the read distance of overlapping neighbours inside the skip loop
 * wrap in the reference's size_t and wrap here.  With the default max_dp_cells (SIZE_MAX) an unreachable pair whose link has 1 .. max_chain_connection
 * bases therefore still goes to WFA, as in the reference; with a finite max_dp_cells it is refused.
 *
 * Out, dense and in chain order.  Per chain: status, flags, its links links[link_begin .. + n_links) (left tail, connects, right tail, in read
 * order), its kept anchors kept[kept_begin .. + n_kept) (numbers within the set), left_tail_length, longest_attempted_connection (the longest
 * WFA-route CONNECT), anchor_score, seq_begin (= seq_off[link_begin]).  Per link: mode (VGK_WFA_*), route, the exclusive end points
 * (VGK_WFA_NO_NODE / offset 0 where the mode has none), read_begin, length, graph_distance (a tail's own length; UINT32_MAX unreachable), chain.
 * EMPTY links are written, with length 0: a link stands between any two kept anchors.  seqs (nullable, then seq_off and seq_cap are unread): the
 * links' bases back to back, link i = seqs[seq_off[i] .. seq_off[i + 1]), as ChainStageInput wants them.
 *
 * Room, the caller's: results n_chains; links link_cap (seq_off link_cap + 1), at most the sum of n_items + 1; kept kept_cap, at most the sum of
 * n_items; seqs seq_cap, at most the sum of the chains' reads' lengths.  VGK_EOPS when a capacity is short: written[0..2] = links, kept anchors,
 * sequence bytes needed, and nothing else is written.  VGK_ETOOBIG, before anything is allocated, when one of those bounds (summed in 64 bits), the
 * reads, anchors, items or distances exceed 2^32 - 16.
 * Per chain VGK_EINVAL, every other field 0, the rest of the call answers: no items; items beyond `items`; an item outside the set; items not
 * ascending by read_start; a kept anchor that ends past its read; an item whose end_offset is 0; a set whose distances do not ascend strictly or
 * name anchors outside it.  For the call VGK_EINVAL: offsets that do not ascend from 0, a read or set number outside the batch.  No chains: VGK_OK. */
enum { VGK_CHAIN_ROUTE_WFA = 0, VGK_CHAIN_ROUTE_DP = 1, VGK_CHAIN_ROUTE_EMPTY = 2, VGK_CHAIN_ROUTE_SOFTCLIP = 3 };
enum { VGK_CHAIN_SITE_SKIPPABLE = 1 };    /* vgk_chain_site.flags */
enum { VGK_CHAIN_LINKS_CUT = 1 };         /* vgk_chain_links_result.flags: the chain ends at a refused link */
typedef struct vgk_chain_site { uint32_t start_node, start_offset, end_node, end_offset, flags; } vgk_chain_site;                 /* 20 B */
typedef struct vgk_chain_links_scheme {   /* MinimizerMapper's fields of the same names; its defaults in brackets */
    uint64_t max_chain_connection;        /* [100] */
    uint64_t max_tail_length;             /* [100] */
    uint64_t max_middle_dp_length;        /* [2^31 - 1] */
    uint64_t max_tail_dp_length;          /* [30000] */
    uint64_t max_dp_cells;                /* [SIZE_MAX] */
    uint64_t max_skipped_bases;           /* [0] */
    uint64_t min_indel_avoid_bases;       /* [0] */
    int32_t  match, full_length_bonus;    /* [1] [5] */
} vgk_chain_links_scheme;                 /* 64 B */
typedef struct vgk_chain_problem { uint32_t read, anchor_set, item_begin, n_items; } vgk_chain_problem;
typedef struct vgk_chain_links_result {
    int32_t status; uint32_t flags, link_begin, n_links, kept_begin, n_kept, left_tail_length, longest_attempted_connection;
    int64_t anchor_score; uint64_t seq_begin;
} vgk_chain_links_result;                 /* 48 B */
typedef struct vgk_chain_link { uint32_t mode, route, from_node, from_offset, to_node, to_offset, read_begin, length, graph_distance, chain; } vgk_chain_link;   /* 40 B */
int vgk_chain_links(vgk_ctx* ctx, const vgk_chain_links_scheme* scheme, uint32_t n_reads, const char* reads, const uint64_t* read_off,
                    uint32_t n_sets, const uint64_t* anchor_off, const vgk_chain_anchor* anchors, const vgk_chain_site* sites,
                    const uint32_t* items, size_t n_items, const uint64_t* dist_off, const vgk_chain_candidate* dist,
                    uint32_t n_chains, const vgk_chain_problem* chains,
                    vgk_chain_links_result* results /* [n_chains] */, vgk_chain_link* links, size_t link_cap, uint32_t* kept, size_t kept_cap,
                    char* seqs /* nullable */, uint64_t* seq_off /* [link_cap + 1] */, size_t seq_cap, size_t written[3]);
/* Device time (ms) of the last vgk_chain_links call on this context: checks + walk | counts, prefix sums and write-out | sequences */
int vgk_chain_links_last_ms(vgk_ctx* ctx, double ms[3]);

/* ---- a long read's mappings chosen on the device: scores, order, uniqueness ------------------------------------------------------------------------
 * The end of MinimizerMapper::do_alignment_on_chains (the multiplicity fix-up, src/minimizer_mapper_from_chains.cpp:2241-2262, with
 * chain_ranges_are_equivalent :100-191) followed by pick_mappings_from_alignments (:2265-2493): the step between the chain stage, which answers with
 * one composed alignment per chain, and vgk_read_mapq, which wants a read's scores in their final order, a multiplicity per score and an unmapped
 * byte.  No distance index and no zip code is read: the four numbers of a chain's range are GIVEN.  The rule is stated serially in
 * vg_amd/csrc/pick_mappings_device.hpp, which the kernels call; the host shim (vg_amd/host/pick_mappings.cpp: vgh_pick_mappings) states it in the
 * reference's shape and is the checker.  No reference unit test names these loops [PARITY-UNPINNED]: the rule is held to a second statement in
 * tests/test_pick_mappings.py.
 *
 * In.  Reads as `reads` / read_off[n_reads + 1] (read for the generator's seed only; nullable when rng_state is).  rng_state: one uint32 per read
 * in vgk_funnel_*'s convention (0: not made yet), updated in place; NULL: nothing is shuffled.  Read r's chains are chains[chain_off[r] ..
 * chain_off[r + 1]): score_estimate (chain_score_estimates), multiplicity (multiplicity_by_chain) and its range {component =
 * get_distance_index_address(0), flags (VGK_CHAIN_RANGE_ROOT_SNARL: get_code_type(0) == ROOT_SNARL), child_start / child_end = get_rank_in_snarl(1)
 * of the chain's first / last seed, offset_start / offset_end = get_seed_offset of the same two seeds}.  Its alignments are alns[aln_off[r] ..
 * aln_off[r + 1]) in the order do_alignment_on_chains made them: source (a chain of the read, numbered within the read), item_count (the
 * better_or_equal_count its chain's walk passed in, :2142), score (final: no softclip_penalty is applied here) and a vgk_chain_result naming its
 * mappings mappings[mapping_begin .. + n_mappings) in vgk_chain_stitch's layout — per mapping {oriented node or VGK_WFA_NO_NODE, offset, edit_begin,
 * n_edits}, its runs edits[edit_begin .. + n_edits) as length << 2 | VGK_WFA_*.  Only mapping_begin and n_mappings of the result are read.  Two
 * results may name the same mappings.
 *
 * The rule.  Equivalent ranges (:100-191): different components: no; when chain 1 is in a root snarl and child_start1 != child_start2 or
 * child_start1 != child_end1 or child_start2 != child_end2: no; each chain's two offsets swapped into order; disjoint: no; one contains the other:
 * yes; otherwise overlap > min(len1, len2) / 2 (integer division).  count[i] = item_count[i] less one for every j != i with estimate[source[i]] >=
 * estimate[source[j]] and equivalent ranges; multiplicity[i] = chain multiplicity + (count >= A ? (double)count - (double)A : 0.0), A = the read's
 * alignments.  THE WRAP: count is the reference's size_t and wraps below 0 here as there — a best chain with item_count 1 and two equivalent lower
 * chains aligned has count 2^64 - 1 and multiplicity + 2^64 - A.  identity (src/path.cpp:2316-2335) = matched bases / to_length, the length less an
 * insertion that is the path's very first or very last edit (an edit that is both: once), 0.0 when that length is 0.  A mapping's from_length = its
 * match, mismatch and deletion runs; a mapping without a node has none and is never entered into the used set.  The walk is
 * process_until_threshold_a: descending by (double)score + identity — or (double)estimate[source] under VGK_PICK_SORT_BY_CHAIN_SCORE — ties at the top
 * shuffled by the read's generator, threshold 0, min 1, max max_multimaps.  Processed (:2334-2404): score <= 0 fails and does not count; fraction
 * unique = (double)(total - used) / total over its mappings' from_lengths (1.0 when total is 0), used = on oriented nodes of the alignments accepted
 * before it; fraction < min_unique_node_fraction fails and does not count; otherwise its nodes are marked, score and multiplicity are appended and
 * it is a mapping.  Beyond the cut (:2405-2466): the same two filters without marking; survivors append score and multiplicity only.  No mapping:
 * one entry of score 0 and multiplicity 0, unmapped = 1 (:2480-2486).
 *
 * Out.  Per read {status, first, n_scores, n_mappings, unmapped}: picked[first .. + n_scores) (the alignment's number within the read; UINT32_MAX
 * for the unmapped entry), scores[] and multiplicity[] beside it, in walk order; the first n_mappings of them are the mappings; first = aln_off[r]
 * + r.  Per alignment {identity, fraction_unique, fate}: fraction_unique is VGK_PICK_NOT_EVALUATED's bits (a quiet NaN) where score <= 0 kept it
 * from being computed; fate one of VGK_PICK_MAPPING, _BEYOND_CUT, _FAIL_SCORE, _FAIL_UNIQUE.
 * Room: `cap` entries of picked / scores / multiplicity, aln_off[n_reads] + n_reads needed; VGK_EOPS when short, *written = what is needed and
 * nothing else is written.  VGK_ETOOBIG, before anything is allocated, when reads, chains, alignments + reads, mappings, edits or the sum of the
 * alignments' mapping counts (in 64 bits) exceed 2^32 - 16.
 * Per read VGK_EINVAL, every other field 0 and its alignments' verdicts 0, the rest of the call answers: a source outside the read's chains; a
 * result whose mappings, or a mapping of it whose runs, lie outside the arrays; a chain multiplicity that is not finite.  For the call VGK_EINVAL:
 * offsets that do not ascend from 0, unknown flags, max_multimaps 0, a min_unique_node_fraction that is NaN, rng_state without reads.  No reads:
 * VGK_OK.
 * Not here: zip-code decoding of the ranges, softclip_penalty, the chain walk that makes item_count, set_refpos, annotations; the resident form
 * (alignments taken where vgk_chain_stitch left them in HBM) is not built. */
enum { VGK_PICK_SORT_BY_CHAIN_SCORE = 1 };   /* vgk_pick_scheme.flags: sort_by_chain_score */
enum { VGK_CHAIN_RANGE_ROOT_SNARL = 1 };     /* vgk_chain_range.flags */
enum { VGK_PICK_MAPPING = 1, VGK_PICK_BEYOND_CUT = 2, VGK_PICK_FAIL_SCORE = 3, VGK_PICK_FAIL_UNIQUE = 4 };   /* vgk_pick_verdict.fate */
#define VGK_PICK_NOT_EVALUATED 0x7ff8000000000000ull   /* the bits of fraction_unique where it was never evaluated */
typedef struct vgk_pick_scheme { double min_unique_node_fraction; /* [0.0] */ uint32_t max_multimaps; /* [1] */ uint32_t flags; } vgk_pick_scheme;   /* 16 B */
typedef struct vgk_chain_range { uint64_t component; uint32_t flags, child_start, child_end, reserved; uint64_t offset_start, offset_end; } vgk_chain_range;   /* 40 B */
typedef struct vgk_pick_chain { int32_t score_estimate; uint32_t reserved; double multiplicity; vgk_chain_range range; } vgk_pick_chain;            /* 56 B */
typedef struct vgk_pick_alignment { uint32_t source; int32_t score; uint64_t item_count; vgk_chain_result result; } vgk_pick_alignment;             /* 48 B */
typedef struct vgk_pick_result { int32_t status; uint32_t first, n_scores, n_mappings, unmapped, reserved; } vgk_pick_result;                       /* 24 B */
typedef struct vgk_pick_verdict { double identity, fraction_unique; uint32_t fate, reserved; } vgk_pick_verdict;                                    /* 24 B */
int vgk_pick_mappings(vgk_ctx* ctx, const vgk_pick_scheme* scheme, uint32_t n_reads, const char* reads /* nullable */, const uint64_t* read_off,
                      uint32_t* rng_state /* nullable */, const uint64_t* chain_off, const vgk_pick_chain* chains, const uint64_t* aln_off,
                      const vgk_pick_alignment* alns, const vgk_chain_mapping* mappings, size_t n_mappings, const uint32_t* edits, size_t n_edits,
                      vgk_pick_result* results /* [n_reads] */, vgk_pick_verdict* verdicts /* [aln_off[n_reads]] */, uint32_t* picked, int32_t* scores,
                      double* multiplicity, size_t cap, size_t* written);
/* out[0] = distinct oriented nodes a read's accepted alignments may hold (the sum of the mapping counts of its max_multimaps largest alignments)
 * with the used set in LDS, out[1] = the slots of that table (open addressing, linear probing from (node * 2654435761 mod 2^32) >> (32 - log2
 * slots)), out[2] = alignments of a read whose walk order lies in LDS, out[3] = lanes per read in the pick.  Reads beyond out[0] or out[2] run in a
 * second launch over a slab in HBM */
int vgk_pick_mappings_limits(uint32_t out[4]);
/* Device time (ms) of the last vgk_pick_mappings call on this context: checks | statistics | multiplicities and sort scores | the pick */
int vgk_pick_mappings_last_ms(vgk_ctx* ctx, double ms[4]);
/* Reads of the last vgk_pick_mappings call by where the pick ran: in LDS | over the slab | refused by the checks */
int vgk_pick_mappings_last_launches(vgk_ctx* ctx, uint64_t reads[3]);

/* ---- windows of the resident graph, of any read length: the wide route on the device ------------------------------------------------------
 * vgk_gssw_pack_windows (vgk.h) takes what the packed kernels take: at most 1024 DP rows, scores inside 11 bits; a longer window fails the whole
 * pack with VGK_ETOOLONG.  This one-call entry takes windows of any read length and scoring and answers every problem in its own status, as
 * vgk_gssw_align does for explicit graphs.  Results are those of vgk_gssw_align on the induced subgraphs of nodes [first_node, first_node + n_nodes):
 * edges entering from outside are dropped, op.node and end_node count from the window's first node.  Modes: VGK_GSSW_LOCAL and VGK_XDROP_PINNED,
 * each with or without VGK_GSSW_TRACEBACK.  A quality-adjusted context: VGK_EUNSUPPORTED for the call.
 *
 * Windows the packed kernels take run as ONE batch through the window packer, in their original relative order; the others are packed on the
 * device for the wide kernels (four wavefronts per problem, int32 cells) in sub-batches of at most a quarter of the device's memory
 * (VGAMD_MAX_BATCH_BYTES, read per call, overrides).  Any graph vgk_gssw_pack_windows accepts is accepted (tail forests included).
 *
 * Per problem (zeroed result fields, the rest of the call goes ahead): VGK_EINVAL an empty read or window, a window beyond the graph, a read
 * beyond reads_bytes, any other mode; VGK_ETOOLONG read_len >= 65535; VGK_ETOOBIG 2^20 graph columns or more; VGK_EOVERFLOW from the kernels;
 * VGK_EOPS the window's ops do not fit what is left of ops_cap (the score and end cell are still reported).  The ops lie in problem order in
 * `ops`; *ops_written is their number. */
int vgk_gssw_align_windows(vgk_ctx* ctx, const vgk_dgraph* graph, const char* reads, size_t reads_bytes,
                           const vgk_window_problem* problems, uint32_t n,
                           vgk_result* results /* [n] */, vgk_op* ops, size_t ops_cap, size_t* ops_written);
/* The last vgk_gssw_align_windows call on this context: 0 device ms of the wide packing kernels, 1 wide fill ms, 2 wide walk ms, 3 windows that
 * went wide, 4 wide sub-batches, 5 op bytes copied back for the wide windows */
double vgk_gssw_align_windows_last(vgk_ctx* ctx, int which);

#ifdef __cplusplus
}
#endif
#endif
