// Compile-only check of per-sequence parameters in bpvo::VisualOdometrySequences (include/bpvo_hip/vo.hpp).
#include <bpvo_hip/vo.hpp>

int seq_params_surface()
{
  bpvo::AlgorithmParameters p;
  p.numPyramidLevels = 4;
  bpvo::Matrix33 K = {{615.0f, 0.0f, 320.0f, 0.0f, 615.0f, 240.0f, 0.0f, 0.0f, 1.0f}};
  std::vector<bpvo::VisualOdometrySequences::Camera> cams(3, bpvo::VisualOdometrySequences::Camera(K, 0.1f, bpvo::ImageSize(480, 640)));
  std::vector<bpvo::AlgorithmParameters> sweep(3, p);
  sweep[1].lossFunction = BPVO_LOSS_TUKEY;
  sweep[1].maxIterations = 50;
  sweep[2].functionTolerance = 5e-4f;
  sweep[2].minSaliency = 0.05f;
  bpvo::VisualOdometrySequences vos(cams, sweep);
  std::vector<uint8_t> images(3 * 480 * 640);
  std::vector<float> disparities(images.size());
  std::vector<bpvo::Result> all = vos.addFrames(images.data(), disparities.data());
  vos.reset(2);
  bpvo::AlgorithmParameters q = vos.parameters(2);
  q.maxValidDisparity = 64.0f;
  vos.setParameters(2, q);
  return (int) all.size() + vos.parameters(1).maxIterations + (int) vos.parameters(2).maxValidDisparity;
}
