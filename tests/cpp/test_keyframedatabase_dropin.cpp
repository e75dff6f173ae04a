// KeyFrameDatabaseT (csrc/compat/orbslam_keyframedatabase.h) over the mock data model: runs the program tests/test_gpu_kfdb_dropin.py writes -
// keyframes with their BowVectors and covisibility lists, then add / erase / clear and the two kinds of query, as LoopClosing, Tracking and
// KeyFrame::SetBadFlag make them - and prints, per query, the returned keyframes and the query fields of every keyframe.  The Python side
// compares with the restatement.
//   program lines:  V n_words | K id n (word value)* | C id n (id)* | A id | E id | X | L id minScore | R frame_id n (word value)*
//   (values as C hexadecimal floats)
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <map>

#include "mock_kfdb.h"
#include "../../ceres_mono_orb_slam2_amd/csrc/compat/orbslam_keyframedatabase.h"

float mock::Frame::fx_, mock::Frame::fy_, mock::Frame::cx_, mock::Frame::cy_, mock::Frame::min_x_, mock::Frame::max_x_, mock::Frame::min_y_, mock::Frame::max_y_;
unsigned long mock::KeyFrame::next_id_ = 0, mock::MapPoint::next_id_ = 0;

typedef KeyFrameDatabaseT<mock::KfdbTypes> KeyFrameDatabase;

static uint32_t bits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }

int main(int argc, char** argv) {
  if (argc < 2) return 2;
  FILE* f = std::fopen(argv[1], "r");
  if (!f) return 2;
  mock::KfdbVocabulary voc;
  KeyFrameDatabase* db = nullptr;
  std::map<long, mock::KfdbKeyFrame*> kfs;
  auto read_bow = [&](mock::BowVector& bow) {
    int n; if (std::fscanf(f, "%d", &n) != 1) return false;
    for (int i = 0; i < n; i++) { unsigned w; double v; if (std::fscanf(f, "%u %la", &w, &v) != 2) return false; bow[w] = v; }
    return true;
  };
  auto dump = [&](const std::vector<mock::KfdbKeyFrame*>& out) {
    std::printf("Q %zu", out.size());
    for (auto* k : out) std::printf(" %lu", k->id_);
    std::printf("\n");
    for (auto& e : kfs) {
      mock::KfdbKeyFrame* k = e.second;
      std::printf("F %ld %lu %d %" PRIu32 " %lu %d %" PRIu32 " %d\n", e.first, k->n_loop_query_, k->n_loop_words_, bits(k->loop_score_), k->reloc_query_, k->n_reloc_words_,
                  bits(k->reloc_score_), k->n_best_calls_);
    }
  };
  char op[8];
  try {
    while (std::fscanf(f, "%7s", op) == 1) {
      long id = 0;
      if (op[0] == 'V') { if (std::fscanf(f, "%u", &voc.n_words) != 1) return 3; db = new KeyFrameDatabase(voc); }
      else if (op[0] == 'X') db->clear();
      else if (op[0] == 'R') {
        mock::KfdbFrame frame;
        if (std::fscanf(f, "%lu", &frame.id_) != 1 || !read_bow(frame.bow_vector_)) return 3;
        dump(db->DetectRelocalizationCandidates(&frame));
      } else {
        if (std::fscanf(f, "%ld", &id) != 1) return 3;
        if (op[0] == 'K') { auto* k = new mock::KfdbKeyFrame(); k->id_ = (unsigned long)id; if (!read_bow(k->bow_vector_)) return 3; kfs[id] = k; }
        else if (op[0] == 'C') {
          int n; if (std::fscanf(f, "%d", &n) != 1) return 3;
          kfs[id]->ordered_.clear();
          for (int i = 0; i < n; i++) { long j; if (std::fscanf(f, "%ld", &j) != 1) return 3; kfs[id]->ordered_.push_back(kfs[j]); }
        }
        else if (op[0] == 'A') db->add(kfs[id]);
        else if (op[0] == 'E') db->erase(kfs[id]);
        else if (op[0] == 'L') { float ms; if (std::fscanf(f, "%a", &ms) != 1) return 3; dump(db->DetectLoopCandidates(kfs[id], ms)); }
        else return 3;
      }
    }
  } catch (const std::exception& e) { std::printf("EXCEPTION %s\n", e.what()); return 4; }
  delete db;
  std::fclose(f);
  std::printf("OK\n");
  return 0;
}
