// Compile-only check of the normalised intensity in the facade (include/bpvo_hip/vo.hpp, config_file.hpp): setIntensityNormalization /
// intensityNormalization on every class that owns or shares a context, and the key of the .cfg files.
#include <bpvo_hip/vo.hpp>
#include <bpvo_hip/config_file.hpp>

int intensity_normalization_surface(const std::string& cfg)
{
  bpvo::AlgorithmParameters p = bpvo::AlgorithmParametersFromFile(cfg);
  const int radius = bpvo::IntensityNormalizationRadiusFromFile(cfg);
  bpvo::Matrix33 K = {{153.75f, 0.0f, 80.0f, 0.0f, 153.75f, 60.0f, 0.0f, 0.0f, 1.0f}};
  const bpvo::ImageSize size(120, 160);

  bpvo::VisualOdometry vo(K, 0.1f, size, p);
  vo.setIntensityNormalization(radius);
  int sum = vo.intensityNormalization();

  typedef bpvo::VisualOdometrySequences::Camera SeqCamera;
  bpvo::VisualOdometrySequences vos(std::vector<SeqCamera>(2, SeqCamera(K, 0.1f, size)), std::vector<bpvo::AlgorithmParameters>(2, p));
  vos.setIntensityNormalization(7);
  sum += vos.intensityNormalization();

  bpvo::Matrix44 I;
  I.fill(0.0f);
  I[0] = I[5] = I[10] = I[15] = 1.0f;
  typedef bpvo::RigVisualOdometry::Camera RigCamera;
  bpvo::RigVisualOdometry rig(std::vector<RigCamera>(2, RigCamera(K, 0.1f, size)), std::vector<bpvo::Matrix44>(2, I), p);
  rig.setIntensityNormalization(0);
  sum += rig.intensityNormalization();

  typedef bpvo::RigsVisualOdometry::Camera RigsCamera;
  std::vector<std::vector<RigsCamera> > cams(2, std::vector<RigsCamera>(2, RigsCamera(K, 0.1f, size)));
  std::vector<std::vector<bpvo::Matrix44> > extrinsics(2, std::vector<bpvo::Matrix44>(2, I));
  bpvo::RigsVisualOdometry rigs(cams, extrinsics, p);
  rigs.setIntensityNormalization(15);
  sum += rigs.intensityNormalization();

  std::shared_ptr<bpvo::detail::Device> dev = std::make_shared<bpvo::detail::Device>(K, 0.1f, size, p, 2, 1);
  bpvo::VisualOdometryFrame frame(dev, 0);
  bpvo::VisualOdometryPoseEstimator estimator(dev);
  frame.setIntensityNormalization(7);
  estimator.setIntensityNormalization(-1);
  return sum + frame.intensityNormalization() + estimator.intensityNormalization();
}
