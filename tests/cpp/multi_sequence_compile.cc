// Compile-only check of bpvo::VisualOdometrySequences (include/bpvo_hip/vo.hpp): many independent VisualOdometry sequences in one context.
#include <bpvo_hip/vo.hpp>

int multi_sequence_surface()
{
  bpvo::AlgorithmParameters p;
  p.numPyramidLevels = 2;
  bpvo::Matrix33 K;
  bpvo::VisualOdometrySequences vos(K, 0.1f, bpvo::ImageSize(64, 64), 4, p);
  const int S = vos.numSequences();
  std::vector<uint8_t> images(4 * 64 * 64);
  std::vector<float> disparities(4 * 64 * 64);
  std::vector<bpvo::Result> all = vos.addFrames(images.data(), disparities.data());               // sequences 0 .. S-1
  const int ids[2] = {3, 1};
  std::vector<bpvo::Result> some = vos.addFrames(images.data(), disparities.data(), ids, 2);      // a subset, in any order
  int acc = S + (int) all.size() + (int) some.size();
  for(const bpvo::Result& r : some) {
    acc += (int) r.isKeyFrame + (int) r.optimizerStatistics.size();
    if(r.pointCloud) acc += (int) r.pointCloud->points().size();
  }
  acc += (int) vos.trajectory(1).poses().size() + vos.numPointsAtLevel(3) + vos.numPointsAtLevel(0, 1);
  vos.reset(2);
  vos.setOption("persistent", 1.0);
  acc += (int) vos.getOption("persistent");
  return acc;
}
