// Compile-only check of the start policy in the facade (include/bpvo_hip/vo.hpp): setStartPolicy, setStartHints and startInfo on every
// VisualOdometry flavour.
#include <bpvo_hip/vo.hpp>

int start_policy_surface()
{
  bpvo::AlgorithmParameters p;
  p.numPyramidLevels = 3;
  bpvo::Matrix33 K = {{153.75f, 0.0f, 80.0f, 0.0f, 153.75f, 60.0f, 0.0f, 0.0f, 1.0f}};
  const bpvo::ImageSize size(120, 160);
  bpvo::Matrix44 I;
  I.fill(0.0f);
  I[0] = I[5] = I[10] = I[15] = 1.0f;
  const std::vector<bpvo::Matrix44> hints(2, I);
  const bpvo::StartPolicy scored(bpvo::StartPolicy::kScored, 0.5f, 2), velocity(bpvo::StartPolicy::kConstantVelocity), reference;

  bpvo::VisualOdometry vo(K, 0.1f, size, p);
  vo.setStartPolicy(scored);
  vo.setStartHints(hints);
  int n = vo.startInfo().n_candidates + vo.startInfo(1).chosen;

  typedef bpvo::VisualOdometrySequences::Camera SeqCamera;
  bpvo::VisualOdometrySequences vos(std::vector<SeqCamera>(2, SeqCamera(K, 0.1f, size)), std::vector<bpvo::AlgorithmParameters>(2, p));
  vos.setStartPolicy(velocity);
  vos.setStartPolicy(1, scored);
  vos.setStartHints(1, hints);
  n += vos.startInfo(1).n_candidates + vos.startInfo(0, 1).kind[0];

  typedef bpvo::RigVisualOdometry::Camera RigCamera;
  bpvo::RigVisualOdometry rig(std::vector<RigCamera>(2, RigCamera(K, 0.1f, size)), std::vector<bpvo::Matrix44>(2, I), p);
  rig.setStartPolicy(scored);
  rig.setStartHints(hints);
  n += rig.startInfo().n_candidates + (int) rig.startInfo(1).scores[0].n_valid;

  typedef bpvo::RigsVisualOdometry::Camera RigsCamera;
  std::vector<std::vector<RigsCamera> > cams(2, std::vector<RigsCamera>(2, RigsCamera(K, 0.1f, size)));
  std::vector<std::vector<bpvo::Matrix44> > extrinsics(2, std::vector<bpvo::Matrix44>(2, I));
  bpvo::RigsVisualOdometry rigs(cams, extrinsics, p);
  rigs.setStartPolicy(reference);
  rigs.setStartPolicy(1, scored);
  rigs.setStartHints(1, hints);
  n += rigs.startInfo(1).n_candidates + (int) rigs.startInfo(0, 1).T_start[0];
  return n;
}
