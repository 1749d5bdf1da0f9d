// The rectification surface of include/bpvo_hip/vo.hpp, compiled and run by tests/test_gpu_rectify.py:
//   rectify_facade <dir> <rows> <cols> <fx> <fy> <cx> <cy> <baseline> <n_sequences> <n_frames> <number_of_disparities>
// reads <dir>/lens.bin (per sequence and side a bpvo_hip_lens: [n_sequences][2]) and, per frame k, <dir>/left_k.u8 and <dir>/right_k.u8 (the raw
// images of the sequences back to back); VisualOdometrySequences::setRectification for every side, then addFramesRaw per frame.  Writes
// <dir>/poses.bin ([n_frames][n_sequences][16] f32) and, per frame and sequence, "isKeyFrame points-in-cloud" to stdout.  Sequence 0 alone then
// goes through VisualOdometry::setRectification / addFrameRaw: <dir>/poses_single.bin ([n_frames][16]).
#include <bpvo_hip/vo.hpp>

#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>

template <class T>
static std::vector<T> read_file(const std::string& path, size_t count)
{
  std::vector<T> v(count);
  std::ifstream f(path.c_str(), std::ios::binary);
  f.read(reinterpret_cast<char*>(v.data()), (std::streamsize) (count * sizeof(T)));
  if((size_t) f.gcount() != count * sizeof(T)) { std::fprintf(stderr, "short read: %s\n", path.c_str()); std::exit(3); }
  return v;
}

int main(int argc, char** argv)
{
  if(argc < 12) { std::fprintf(stderr, "arguments: see the head of this file\n"); return 2; }
  const std::string dir = argv[1];
  const int rows = std::atoi(argv[2]), cols = std::atoi(argv[3]);
  const bpvo::Matrix33 K = {{(float) std::atof(argv[4]), 0.0f, (float) std::atof(argv[6]), 0.0f, (float) std::atof(argv[5]), (float) std::atof(argv[7]), 0.0f, 0.0f, 1.0f}};
  const float baseline = (float) std::atof(argv[8]);
  const int S = std::atoi(argv[9]), n_frames = std::atoi(argv[10]);
  bpvo::AlgorithmParameters p;
  p.numPyramidLevels = 3;
  p.descriptor = BPVO_DESC_BITPLANES;
  p.lossFunction = BPVO_LOSS_TUKEY;
  p.verbosity = BPVO_VERB_SILENT;
  const bpvo::StereoParameters stereo(std::atoi(argv[11]));
  try {
    const std::vector<bpvo_hip_lens> lens = read_file<bpvo_hip_lens>(dir + "/lens.bin", (size_t) 2 * S);
    size_t raw_left = 0, raw_right = 0;
    for(int s = 0; s < S; ++s) {
      raw_left += (size_t) lens[2 * s].raw_rows * lens[2 * s].raw_cols;
      raw_right += (size_t) lens[2 * s + 1].raw_rows * lens[2 * s + 1].raw_cols;
    }
    bpvo::VisualOdometrySequences vo(K, baseline, bpvo::ImageSize(rows, cols), S, p);
    for(int s = 0; s < S; ++s)
      for(int side = 0; side < 2; ++side) vo.setRectification(s, side, lens[2 * s + side]);
    bpvo::VisualOdometry single(K, baseline, bpvo::ImageSize(rows, cols), p);
    for(int side = 0; side < 2; ++side) single.setRectification(side, lens[side]);
    std::ofstream poses(dir + "/poses.bin", std::ios::binary), poses_single(dir + "/poses_single.bin", std::ios::binary);
    for(int k = 0; k < n_frames; ++k) {
      const std::vector<uint8_t> left = read_file<uint8_t>(dir + "/left_" + std::to_string(k) + ".u8", raw_left);
      const std::vector<uint8_t> right = read_file<uint8_t>(dir + "/right_" + std::to_string(k) + ".u8", raw_right);
      const std::vector<bpvo::Result> res = vo.addFramesRaw(left.data(), right.data(), stereo);
      for(int s = 0; s < S; ++s) {
        poses.write(reinterpret_cast<const char*>(res[(size_t) s].pose.data()), 16 * sizeof(float));
        std::printf("%d %zu\n", res[(size_t) s].isKeyFrame ? 1 : 0, res[(size_t) s].pointCloud ? res[(size_t) s].pointCloud->size() : (size_t) 0);
      }
      const bpvo::Result one = single.addFrameRaw(left.data(), right.data(), stereo);      // (sequence 0's pair comes first in both buffers)
      poses_single.write(reinterpret_cast<const char*>(one.pose.data()), 16 * sizeof(float));
    }
  } catch(const std::exception& e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
  return 0;
}
