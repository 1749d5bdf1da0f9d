// Compile-only check of per-sequence cameras in bpvo::VisualOdometrySequences (include/bpvo_hip/vo.hpp).
#include <bpvo_hip/vo.hpp>

int seq_cameras_surface()
{
  bpvo::AlgorithmParameters p;
  p.numPyramidLevels = 4;
  bpvo::Matrix33 K = {{615.0f, 0.0f, 320.0f, 0.0f, 615.0f, 240.0f, 0.0f, 0.0f, 1.0f}};
  std::vector<bpvo::VisualOdometrySequences::Camera> cams;
  cams.push_back(bpvo::VisualOdometrySequences::Camera(K, 0.1f, bpvo::ImageSize(480, 640)));
  cams.push_back(bpvo::VisualOdometrySequences::Camera(K, 0.12f, bpvo::ImageSize(474, 632)));
  bpvo::VisualOdometrySequences vos(cams, p);
  std::vector<uint8_t> images(480 * 640 + 474 * 632);
  std::vector<float> disparities(images.size());
  std::vector<bpvo::Result> all = vos.addFrames(images.data(), disparities.data());      // frame 0: 480 x 640, frame 1: 474 x 632
  vos.reset(1);
  vos.setCamera(1, bpvo::VisualOdometrySequences::Camera(K, 0.14f, bpvo::ImageSize(462, 616)));
  const bpvo::VisualOdometrySequences::Camera c = vos.camera(1);
  return (int) all.size() + c.size.rows + (int) c.baseline;
}
