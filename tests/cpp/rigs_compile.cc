// Compile-and-link check of bpvo::RigsVisualOdometry (include/bpvo_hip/vo.hpp): every member function instantiated.
#include <bpvo_hip/vo.hpp>

int rigs_surface()
{
  bpvo::AlgorithmParameters p;
  p.numPyramidLevels = 3;
  bpvo::Matrix33 K = {{153.75f, 0.0f, 80.0f, 0.0f, 153.75f, 60.0f, 0.0f, 0.0f, 1.0f}};
  typedef bpvo::RigsVisualOdometry::Camera Camera;
  std::vector<std::vector<Camera> > cams(2, std::vector<Camera>(2, Camera(K, 0.1f, bpvo::ImageSize(120, 160))));
  bpvo::Matrix44 I;
  I.fill(0.0f);
  I[0] = I[5] = I[10] = I[15] = 1.0f;
  std::vector<std::vector<bpvo::Matrix44> > extrinsics(2, std::vector<bpvo::Matrix44>(2, I));
  extrinsics[0][1][3] = 0.3f;
  extrinsics[1][1][3] = -0.3f;
  bpvo::RigsVisualOdometry rigs(cams, extrinsics, p);
  bpvo::AlgorithmParameters own = rigs.parameters(1);
  own.maxIterations = 5;
  rigs.setParameters(1, own);
  rigs.setPoseCovariance(true);
  std::vector<uint8_t> images(4 * 120 * 160);
  std::vector<float> disparities(images.size());
  std::vector<bpvo::Result> r = rigs.addFrames(images.data(), disparities.data());
  const int only[1] = {1};
  r = rigs.addFrames(images.data(), disparities.data(), only, 1);
  int n = rigs.numRigs() + rigs.numCameras(0) + (int) rigs.trajectory(1).size() + rigs.numPointsAtLevel(1, 0) + rigs.poseCovariance(1).status;
  if(rigs.hasPointClouds(1)) n += (int) rigs.pointCloud(1, 1).size();
  return n + (r[0].isKeyFrame ? 1 : 0) + (int) rigs.getOption("pose_covariance");
}

int main(int argc, char**)
{
  return argc > 100 ? rigs_surface() : 0;      // (linked, never run: there may be no device)
}
