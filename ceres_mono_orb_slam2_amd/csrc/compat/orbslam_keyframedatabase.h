// ============================================================================
// orbslam_keyframedatabase.h -- ORB_SLAM2::KeyFrameDatabase over the HIP C ABI (orbv_db_*, include/orbslam_hip.h): the reference's
// interface (include/KeyFrameDatabase.h) - constructor from the vocabulary, add, erase, clear, DetectLoopCandidates(KeyFrame*, float),
// DetectRelocalizationCandidates(Frame*) - with the inverted file replaced by the device-resident database.
//
// The class is a template over a types bundle (KeyFrame, Frame, ORBVocabulary), as the other drop-in headers are:
//     #define ORBSLAM_DROPIN_REFERENCE_TYPES      (before including this header; needs KeyFrame.h, Frame.h, ORBVocabulary.h)
// makes ORB_SLAM2::KeyFrameDatabase = KeyFrameDatabaseT<KeyFrameDatabaseReferenceTypes>; src/KeyFrameDatabase.cc drops out of the build.
// tests/cpp/ instantiates it over the mock data model.
//
// What is kept of the reference, beyond the returned vectors (same keyframes, same order):
//   * keyframe->id_ / frame->id_ are the query stamps.  The library wants them positive and increasing per kind of query - which every
//     call the reference makes satisfies (DetectLoop returns before the query for the first ten keyframe ids; frame ids grow) - and
//     a call that breaks the rule throws instead of comparing against a stamp that was never set.
//   * n_loop_query_ / n_loop_words_ / loop_score_ and reloc_query_ / n_reloc_words_ / reloc_score_ of every keyframe the query stamped are
//     written back, so code that reads them keeps working.  (A keyframe connected to a loop query is not stamped by the reference
//     either; its n_loop_words_, which the reference leaves at a meaningless 1, is not touched here.)
//   * GetBestCovisibilityKeyFrames(10) is asked of the kept keyframes only (score_and_matches), between the two halves of the query.
// What differs: the reference holds mutex_ over the walk of the inverted file only.  Here the walk, the scores and the selection are one
// pending device query, and add / erase would cancel it, so mutex_ is held from the first half to the second (well under a millisecond).
// GetBestCovisibilityKeyFrames runs under it; it takes the keyframe's own connection mutex, which no path of the reference holds while it
// calls into the database.  A keyframe keeps its slot for the lifetime of the database (erase and add again: same slot, and - as the
// object's fields in the reference - the same relocalisation state); clear() starts afresh.
// ============================================================================
#pragma once
#include <cstdint>
#include <map>
#include <mutex>
#include <set>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../../include/orbslam_hip.h"

template <class Types>
class KeyFrameDatabaseT {
 public:
  typedef typename Types::KeyFrame KeyFrame;
  typedef typename Types::Frame Frame;
  typedef typename Types::ORBVocabulary ORBVocabulary;

  KeyFrameDatabaseT(const ORBVocabulary& voc, int device = 0) : orb_vocabulary_(&voc) {
    check(orbv_db_create((int)voc.size(), device, &db_), "orbv_db_create");
  }
  ~KeyFrameDatabaseT() { orbv_db_destroy(db_); }
  KeyFrameDatabaseT(const KeyFrameDatabaseT&) = delete;
  KeyFrameDatabaseT& operator=(const KeyFrameDatabaseT&) = delete;

  void add(KeyFrame* keyframe) {
    std::unique_lock<std::mutex> lock(mutex_);
    std::vector<uint32_t> w; std::vector<double> v;
    flatten(keyframe->bow_vector_, w, v);
    check(orbv_db_add(db_, slot_of(keyframe), w.data(), v.data(), (int)w.size()), "orbv_db_add");
  }

  void erase(KeyFrame* keyframe) {
    std::unique_lock<std::mutex> lock(mutex_);
    auto it = slots_.find(keyframe);
    if (it != slots_.end()) check(orbv_db_erase(db_, it->second), "orbv_db_erase");
  }

  void clear() {
    std::unique_lock<std::mutex> lock(mutex_);
    check(orbv_db_clear(db_), "orbv_db_clear");
    slots_.clear(); keyframes_.clear();
  }

  std::vector<KeyFrame*> DetectLoopCandidates(KeyFrame* keyframe, float minScore) {
    auto connected_keyframes = keyframe->GetConnectedKeyFrames();
    std::unique_lock<std::mutex> lock(mutex_);
    std::vector<int32_t> connected;
    for (KeyFrame* kf : connected_keyframes) { auto it = slots_.find(kf); if (it != slots_.end()) connected.push_back(it->second); }
    std::vector<uint32_t> w; std::vector<double> v;
    flatten(keyframe->bow_vector_, w, v);
    std::vector<int32_t> kept(keyframes_.size() + 1); int32_t n_kept = 0;
    check(orbv_db_detect_loop_candidates_begin(db_, w.data(), v.data(), (int)w.size(), connected.data(), (int)connected.size(), minScore, (int64_t)keyframe->id_,
                                               kept.data(), (int)kept.size(), &n_kept), "orbv_db_detect_loop_candidates_begin");
    kept.resize(n_kept);
    write_back(true, (long unsigned int)keyframe->id_);
    return finish(kept);
  }

  std::vector<KeyFrame*> DetectRelocalizationCandidates(Frame* frame) {
    std::unique_lock<std::mutex> lock(mutex_);
    std::vector<uint32_t> w; std::vector<double> v;
    flatten(frame->bow_vector_, w, v);
    std::vector<int32_t> kept(keyframes_.size() + 1); int32_t n_kept = 0;
    check(orbv_db_detect_relocalization_candidates_begin(db_, w.data(), v.data(), (int)w.size(), (int64_t)frame->id_, kept.data(), (int)kept.size(), &n_kept),
          "orbv_db_detect_relocalization_candidates_begin");
    kept.resize(n_kept);
    write_back(false, (long unsigned int)frame->id_);
    return finish(kept);
  }

 protected:
  static void check(int rc, const char* what) {
    if (rc != 0) throw std::runtime_error(std::string(what) + " failed: " + orbhip_last_error());
  }
  template <class Bow> static void flatten(const Bow& bow, std::vector<uint32_t>& w, std::vector<double>& v) {     // std::map order = ascending word id
    w.clear(); v.clear();
    for (auto it = bow.begin(); it != bow.end(); ++it) { w.push_back((uint32_t)it->first); v.push_back((double)it->second); }
  }
  int slot_of(KeyFrame* kf) {
    auto it = slots_.find(kf);
    if (it != slots_.end()) return it->second;
    const int s = (int)keyframes_.size();
    slots_[kf] = s; keyframes_.push_back(kf);
    return s;
  }
  // the fields of the keyframes the pending query stamped
  void write_back(bool loop, long unsigned int id) {
    const int S = (int)keyframes_.size();
    if (S == 0) return;
    std::vector<int32_t> words(S); std::vector<float> score(S); orbv_db_query_info info;
    check(orbv_db_pending_fields(db_, &info, words.data(), score.data(), S), "orbv_db_pending_fields");
    for (int s = 0; s < S; s++) {
      if (words[s] <= 0) continue;
      KeyFrame* kf = keyframes_[s];
      if (loop) { kf->n_loop_query_ = id; kf->n_loop_words_ = words[s]; if (words[s] > info.min_common) kf->loop_score_ = score[s]; }
      else { kf->reloc_query_ = id; kf->n_reloc_words_ = words[s]; if (words[s] > info.min_common) kf->reloc_score_ = score[s]; }
    }
  }
  std::vector<KeyFrame*> finish(const std::vector<int32_t>& kept) {
    std::vector<int32_t> rows(kept.size() * 10 + 1, 0), row_n(kept.size() + 1, 0);
    for (size_t i = 0; i < kept.size(); i++) {
      auto neighs = keyframes_[kept[i]]->GetBestCovisibilityKeyFrames(10);
      int n = 0;
      for (KeyFrame* kf : neighs) {
        auto it = slots_.find(kf);
        if (it != slots_.end() && n < 10) rows[i * 10 + n++] = it->second;      // (a neighbour the database has never seen contributes nothing)
      }
      row_n[i] = n;
    }
    std::vector<int32_t> cand(kept.size() * 11 + 1); int32_t n_cand = 0;      // a candidate is a kept keyframe or one of its neighbours
    check(orbv_db_detect_candidates_finish(db_, rows.data(), row_n.data(), cand.data(), (int)cand.size(), &n_cand, nullptr), "orbv_db_detect_candidates_finish");
    std::vector<KeyFrame*> out;
    out.reserve(n_cand);
    for (int i = 0; i < n_cand; i++) out.push_back(keyframes_[cand[i]]);
    return out;
  }

  const ORBVocabulary* orb_vocabulary_;
  orbv_db* db_ = nullptr;
  std::map<KeyFrame*, int> slots_;
  std::vector<KeyFrame*> keyframes_;
  std::mutex mutex_;
};

#ifdef ORBSLAM_DROPIN_REFERENCE_TYPES
// Inside the reference tree (KeyFrame.h, Frame.h, ORBVocabulary.h already included): the class Tracking, LoopClosing, KeyFrame and System name.
namespace ORB_SLAM2 {
struct KeyFrameDatabaseReferenceTypes {
  typedef ORB_SLAM2::KeyFrame KeyFrame; typedef ORB_SLAM2::Frame Frame; typedef ORB_SLAM2::ORBVocabulary ORBVocabulary;
};
typedef KeyFrameDatabaseT<KeyFrameDatabaseReferenceTypes> KeyFrameDatabase;
}  // namespace ORB_SLAM2
#endif
