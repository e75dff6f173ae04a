// What the KeyFrameDatabase drop-in tests need beside mock_orbslam.h: a keyframe with GetConnectedKeyFrames and the six query fields of the
// reference's KeyFrame (include/KeyFrame.h: n_loop_query_, n_loop_words_, loop_score_, reloc_query_, n_reloc_words_, reloc_score_), a frame with
// an id, a vocabulary with size(), and the types bundle KeyFrameDatabaseT takes.
#pragma once
#include <set>
#include <vector>

#include "mock_orbslam.h"

namespace mock {

struct KfdbKeyFrame : KeyFrame {
  long unsigned int n_loop_query_ = 0; int n_loop_words_ = 0; float loop_score_ = 0.0f;
  long unsigned int reloc_query_ = 0; int n_reloc_words_ = 0; float reloc_score_ = 0.0f;
  std::vector<KfdbKeyFrame*> ordered_;                      // the covisibility graph of this keyframe, best first
  int n_best_calls_ = 0;
  std::set<KfdbKeyFrame*> GetConnectedKeyFrames() { return std::set<KfdbKeyFrame*>(ordered_.begin(), ordered_.end()); }
  std::vector<KfdbKeyFrame*> GetBestCovisibilityKeyFrames(const int& N) {
    n_best_calls_++;
    if ((int)ordered_.size() < N) return ordered_;
    return std::vector<KfdbKeyFrame*>(ordered_.begin(), ordered_.begin() + N);
  }
};

struct KfdbFrame : Frame { long unsigned int id_ = 0; };

struct KfdbVocabulary { unsigned int n_words = 0; unsigned int size() const { return n_words; } };

struct KfdbTypes { typedef KfdbKeyFrame KeyFrame; typedef KfdbFrame Frame; typedef KfdbVocabulary ORBVocabulary; };

}  // namespace mock
