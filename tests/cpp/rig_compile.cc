// Compile-only check of bpvo::RigVisualOdometry (include/bpvo_hip/vo.hpp).
#include <bpvo_hip/vo.hpp>

int rig_surface()
{
  bpvo::AlgorithmParameters p;
  p.numPyramidLevels = 3;
  bpvo::Matrix33 K = {{153.75f, 0.0f, 80.0f, 0.0f, 153.75f, 60.0f, 0.0f, 0.0f, 1.0f}};
  std::vector<bpvo::RigVisualOdometry::Camera> cams(2, bpvo::RigVisualOdometry::Camera(K, 0.1f, bpvo::ImageSize(120, 160)));
  bpvo::Matrix44 I;
  I.fill(0.0f);
  I[0] = I[5] = I[10] = I[15] = 1.0f;
  std::vector<bpvo::Matrix44> extrinsics(2, I);
  extrinsics[1][3] = 0.3f;
  bpvo::RigVisualOdometry rig(cams, extrinsics, p);
  std::vector<uint8_t> images(2 * 120 * 160);
  std::vector<float> disparities(images.size());
  bpvo::Result r = rig.addFrame(images.data(), disparities.data());
  int n = (int) rig.trajectory().size() + rig.numCameras() + rig.numPointsAtLevel(1);
  if(rig.hasPointClouds()) n += (int) rig.pointCloud(1).size();
  return n + (r.isKeyFrame ? 1 : 0);
}
