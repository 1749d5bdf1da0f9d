// Compile-only check of the stereo overload of bpvo::VisualOdometrySequences::addFrames (include/bpvo_hip/vo.hpp).
#include <bpvo_hip/vo.hpp>

int stereo_sequences_surface()
{
  bpvo::AlgorithmParameters p;
  p.numPyramidLevels = 4;
  bpvo::Matrix33 K = {{615.0f, 0.0f, 320.0f, 0.0f, 615.0f, 240.0f, 0.0f, 0.0f, 1.0f}};
  std::vector<bpvo::VisualOdometrySequences::Camera> cams;
  cams.push_back(bpvo::VisualOdometrySequences::Camera(K, 0.1f, bpvo::ImageSize(480, 640)));
  cams.push_back(bpvo::VisualOdometrySequences::Camera(K, 0.12f, bpvo::ImageSize(474, 632)));
  bpvo::VisualOdometrySequences vos(cams, p);
  std::vector<uint8_t> left(480 * 640 + 474 * 632), right(left.size());
  std::vector<float> disparities(left.size());
  const bpvo::StereoParameters bm(64);
  std::vector<bpvo::Result> all = vos.addFrames(left.data(), right.data(), bm);      // pair 0: 480 x 640, pair 1: 474 x 632
  const int only[1] = {1};
  std::vector<bpvo::Result> one = vos.addFrames(left.data() + 480 * 640, right.data() + 480 * 640, bpvo::StereoParameters::SemiGlobalMatching(64), only, 1);
  std::vector<bpvo::Result> maps = vos.addFrames(left.data(), disparities.data());      // the disparity overload next to it
  return (int) (all.size() + one.size() + maps.size());
}
