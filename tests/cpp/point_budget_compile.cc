// Compile-only check of the point budget in the facade (include/bpvo_hip/vo.hpp): setPointBudget on every VisualOdometry flavour, both forms.
#include <bpvo_hip/vo.hpp>

int point_budget_surface()
{
  bpvo::AlgorithmParameters p;
  p.numPyramidLevels = 3;
  bpvo::Matrix33 K = {{153.75f, 0.0f, 80.0f, 0.0f, 153.75f, 60.0f, 0.0f, 0.0f, 1.0f}};
  const bpvo::ImageSize size(120, 160);
  std::vector<int> budget(3);
  budget[0] = 4096; budget[1] = 1024; budget[2] = 256;

  bpvo::VisualOdometry vo(K, 0.1f, size, p);
  vo.setPointBudget(budget);
  vo.setPointBudget(8000);

  typedef bpvo::VisualOdometrySequences::Camera SeqCamera;
  bpvo::VisualOdometrySequences vos(std::vector<SeqCamera>(2, SeqCamera(K, 0.1f, size)), std::vector<bpvo::AlgorithmParameters>(2, p));
  vos.setPointBudget(0, budget);
  vos.setPointBudget(1, 8000);
  vos.setPointBudget(0, std::vector<int>());      // back to the context's budget

  bpvo::Matrix44 I;
  I.fill(0.0f);
  I[0] = I[5] = I[10] = I[15] = 1.0f;
  typedef bpvo::RigVisualOdometry::Camera RigCamera;
  bpvo::RigVisualOdometry rig(std::vector<RigCamera>(2, RigCamera(K, 0.1f, size)), std::vector<bpvo::Matrix44>(2, I), p);
  rig.setPointBudget(budget);
  rig.setPointBudget(8000);

  typedef bpvo::RigsVisualOdometry::Camera RigsCamera;
  std::vector<std::vector<RigsCamera> > cams(2, std::vector<RigsCamera>(2, RigsCamera(K, 0.1f, size)));
  std::vector<std::vector<bpvo::Matrix44> > extrinsics(2, std::vector<bpvo::Matrix44>(2, I));
  bpvo::RigsVisualOdometry rigs(cams, extrinsics, p);
  rigs.setPointBudget(budget);
  rigs.setPointBudget(8000);
  return vo.numPointsAtLevel(0) + vos.numSequences() + rig.numCameras() + rigs.numRigs();
}
