/* rumi_kfdb.h — C ABI of the MI355X key-frame database (place recognition and relocalisation).
 *
 * Replaces ORB_SLAM3::KeyFrameDatabase (R/lib_src/KeyFrameDatabase.cc) for the two queries the system calls:
 *   DetectRelocalizationCandidates(Frame*, Map*)                 KeyFrameDatabase.cc:733-843  (Tracking.cc:3219)
 *   DetectNBestCandidates(KeyFrame*, loop&, merge&, N)           KeyFrameDatabase.cc:604-708  (LoopClosing.cc:461, CloudMerging.cc:925)
 * and the members that keep the inverted file: add / erase / clear / clearMap (:38-98).  Scores are DBoW2's L1Scoring::score
 * (Thirdparty/DBoW2/DBoW2/ScoringObject.cpp:23-68); a vocabulary with any other ScoringType is refused (RUMI_E_INVALID).
 *
 * Results equal the reference's for the same database contents and call sequence: the same key-frames in the same order, the
 * float scores bit-equal.  The per-key-frame query state the reference keeps on KeyFrame (mnRelocQuery / mRelocScore and
 * mnPlaceRecognitionQuery / mPlaceRecognitionScore) is kept here per key-frame id, and it survives erase and re-add of the same id
 * (the reference's KeyFrame object survives being taken out of the inverted file).  Its initial value is (query 0, score 0).
 *
 * Key-frame ids are the reference's 64-bit mnId; map ids are caller-chosen int32.  Key-frame BowVectors are (word id strictly
 * ascending, value) arrays, the output of rumi_voc_transform.  Every added key-frame gets the next value of an add sequence
 * (rumi_kfdb_next_seq); a query's visible_below hides key-frames added at or after that sequence value, which lets one batch express
 * "query key-frame b, then add it" for B key-frames (add all B, then query b with visible_below = seq of b).
 *
 * Adds are staged on the host and applied to the device in one batch by the next call of any other entry point.  Every entry point works on
 * the default (null) stream and returns when its results are on the host; rumi_kfdb_add_batch_device first waits for the caller's stream.
 *
 * Between rumi_kfdb_score and the select of the same kind, only rumi_kfdb_scored, rumi_kfdb_set_covisibles, rumi_kfdb_set_maps,
 * rumi_kfdb_set_bad and rumi_kfdb_set_map_bad may be called: the select reads what they set (the model as it is at the end of the query).
 * Status codes as in rumi_orb.h.  No CPU fallback. */
#ifndef RUMI_KFDB_H
#define RUMI_KFDB_H
#include <stdint.h>

#include "rumi_orb.h"
#include "rumi_voc.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct RumiKFDatabase RumiKFDatabase;

enum { RUMI_KFDB_RELOC = 0, RUMI_KFDB_NBEST = 1 };
#define RUMI_KFDB_NCOV 10 /* GetBestCovisibilityKeyFrames(10) */

/* max_kf live key-frames, max_entries live BowVector entries (sum of the live key-frames' word counts, < 2^31).  The vocabulary
 * must outlive the database. */
int rumi_kfdb_create(const RumiVocabulary *voc, int32_t max_kf, int64_t max_entries, int32_t device, RumiKFDatabase **out);
void rumi_kfdb_destroy(RumiKFDatabase *db);
int rumi_kfdb_clear(RumiKFDatabase *db);                     /* KeyFrameDatabase::clear: every key-frame leaves the inverted file */
int32_t rumi_kfdb_size(const RumiKFDatabase *db);            /* live key-frames, staged adds included */
int64_t rumi_kfdb_next_seq(const RumiKFDatabase *db);        /* add sequence value of the next added key-frame */
int32_t rumi_kfdb_max_batch(const RumiKFDatabase *db);       /* most queries one rumi_kfdb_score call takes */

/* KeyFrameDatabase::add for n key-frames in this order: BowVector of key-frame i = (words, values)[offsets[i] .. offsets[i+1]).
 * An id that is already in the database is refused (RUMI_E_INVALID).  RUMI_E_CAPACITY when max_kf or max_entries would be exceeded;
 * nothing is added then. */
int rumi_kfdb_add(RumiKFDatabase *db, int32_t n, const uint64_t *kf_ids, const int32_t *map_ids, const int32_t *offsets,
                  const uint32_t *words, const double *values);
/* The same for the device-resident per-feature output of rumi_voc_transform_batch_device: d_word [nframes][cap] (uint32),
 * d_weight [nframes][cap] (double), d_counts [nframes][2] (n, monoIndex).  The BowVectors are assembled on the device, bit-identical
 * to rumi_voc_assemble: per-word sums in feature order, stopped words (weight <= 0) dropped, the L1 norm summed in word order, one
 * division per entry.  kf_ids / map_ids are host arrays [nframes]. */
int rumi_kfdb_add_batch_device(RumiKFDatabase *db, int32_t nframes, const uint64_t *kf_ids, const int32_t *map_ids, const void *d_word,
                               const void *d_weight, const void *d_counts, int32_t cap, void *hip_stream);
/* The stored BowVector of one key-frame (host arrays of capacity cap). */
int rumi_kfdb_bow(RumiKFDatabase *db, uint64_t kf_id, uint32_t *words, double *values, int32_t cap, int32_t *n_out);

int rumi_kfdb_erase(RumiKFDatabase *db, int32_t n, const uint64_t *kf_ids); /* KeyFrameDatabase::erase (KeyFrame::SetBadFlag, KeyFrame.cc:865); unknown ids are ignored */
int rumi_kfdb_clear_map(RumiKFDatabase *db, int32_t map_id);                /* KeyFrameDatabase::clearMap (Tracking.cc:3442): by each key-frame's current map */
int rumi_kfdb_set_map_bad(RumiKFDatabase *db, int32_t map_id, int32_t bad); /* Map::IsBad, read by the N-best selection */
int rumi_kfdb_set_maps(RumiKFDatabase *db, int32_t n, const uint64_t *kf_ids, const int32_t *map_ids); /* KeyFrame::GetMap changed (map merge) */
int rumi_kfdb_set_bad(RumiKFDatabase *db, int32_t n, const uint64_t *kf_ids, const uint8_t *bad);      /* KeyFrame::isBad, skipped by the N-best walk */
/* GetBestCovisibilityKeyFrames(10) of n key-frames, in its order, padded with -1: best [n][10].  Ids not in the database never
 * contribute. */
int rumi_kfdb_set_covisibles(RumiKFDatabase *db, int32_t n, const uint64_t *kf_ids, const int64_t *best);

/* Stage 1 of nq queries of one kind (at most rumi_kfdb_max_batch), equal to nq reference calls in this order: counts over the inverted
 * file, marks, word threshold, the L1 score of every listed key-frame above it.  query_ids: the Frame's / KeyFrame's mnId, distinct
 * within the call; query_maps: the query's map; visible_below: per-query add-sequence bound, or NULL (no bound).  BowVector of query q =
 * bow_words / bow_vals [bow_off[q] .. bow_off[q+1]).  N-best only: the GetConnectedKeyFrames() set of query q = conn_ids
 * [conn_off[q] .. conn_off[q+1]) (NULL conn_off: empty sets).  Out: scored_off [nq + 1], the CSR of the scored lists (list order).
 * Must be followed by the select of the same kind before the next score. */
int rumi_kfdb_score(RumiKFDatabase *db, int32_t kind, int32_t nq, const uint64_t *query_ids, const int32_t *query_maps,
                    const int64_t *visible_below, const int32_t *bow_off, const uint32_t *bow_words, const double *bow_vals,
                    const int32_t *conn_off, const uint64_t *conn_ids, int32_t *scored_off);
/* The scored (kf id, si) pairs of the pending score call, per query in list order (arrays of scored_off[nq] entries). */
int rumi_kfdb_scored(RumiKFDatabase *db, uint64_t *kf_ids, float *si);
/* Stage 2, relocalisation: covisibility accumulation and DetectRelocalizationCandidates' output, candidates of query q =
 * cand_ids [cand_off[q] .. cand_off[q+1]) (cand_ids capacity cap >= scored_off[nq] suffices). */
int rumi_kfdb_select_reloc(RumiKFDatabase *db, int32_t *cand_off, uint64_t *cand_ids, int64_t cap);
/* Stage 2, N-best: n_cand [nq] (DetectNBestCandidates' nNumCandidates, <= stride); loop_ids / merge_ids [nq][stride], counts n_loop /
 * n_merge [nq]. */
int rumi_kfdb_select_nbest(RumiKFDatabase *db, const int32_t *n_cand, int32_t stride, int32_t *n_loop, uint64_t *loop_ids, int32_t *n_merge,
                           uint64_t *merge_ids);

#ifdef __cplusplus
}
#endif
#endif
