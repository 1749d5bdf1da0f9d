// Compile-only check of the pose-covariance surface of include/bpvo_hip/vo.hpp: setPoseCovariance / poseCovariance on the three VisualOdometry classes.
#include <bpvo_hip/vo.hpp>

int pose_covariance_surface()
{
  bpvo::AlgorithmParameters p;
  p.numPyramidLevels = 2;
  bpvo::Matrix33 K = {{153.75f, 0.0f, 80.0f, 0.0f, 153.75f, 60.0f, 0.0f, 0.0f, 1.0f}};
  std::vector<uint8_t> images(2 * 120 * 160);
  std::vector<float> disparities(images.size());
  int n = 0;

  bpvo::VisualOdometry vo(K, 0.1f, bpvo::ImageSize(120, 160), p);
  vo.setPoseCovariance(true);
  bpvo::Result r = vo.addFrame(images.data(), disparities.data());
  const bpvo::PoseCovarianceEstimate e = vo.poseCovariance();
  n += (e.status == bpvo::PoseCovarianceEstimate::kNone ? 1 : 0) + (r.covariance[0] == e.covariance[0] ? 1 : 0) + e.numValid + e.level + (int) e.sigma + (int) e.pose[0];

  bpvo::VisualOdometrySequences seqs(K, 0.1f, bpvo::ImageSize(120, 160), 2, p);
  seqs.setPoseCovariance(true);
  std::vector<bpvo::Result> rs = seqs.addFrames(images.data(), disparities.data());
  n += (int) rs.size() + (seqs.poseCovariance(1).status == bpvo::PoseCovarianceEstimate::kOk ? 1 : 0);

  std::vector<bpvo::RigVisualOdometry::Camera> cams(2, bpvo::RigVisualOdometry::Camera(K, 0.1f, bpvo::ImageSize(120, 160)));
  bpvo::Matrix44 I;
  I.fill(0.0f);
  I[0] = I[5] = I[10] = I[15] = 1.0f;
  std::vector<bpvo::Matrix44> extrinsics(2, I);
  extrinsics[1][3] = 0.3f;
  bpvo::RigVisualOdometry rig(cams, extrinsics, p);
  rig.setPoseCovariance(true);
  bpvo::Result rr = rig.addFrame(images.data(), disparities.data());
  n += (rig.poseCovariance().status == bpvo::PoseCovarianceEstimate::kIndefinite ? 1 : 0) + (rr.isKeyFrame ? 1 : 0);
  return n;
}
