// The pose-scoring surface of include/bpvo_hip/vo.hpp, compiled and run by tests/test_gpu_pose_score_facade.py:
//   pose_score_facade <dir> <rows> <cols> <fx> <fy> <cx> <cy> <baseline> <n_candidates> <tau> <level> <descriptor: intensity | bitplanes>
// reads <dir>/imgA.u8, dispA.f32, imgB.u8, dispB.f32 and candidates.f32 ([n][16]); writes <dir>/scores.bin (the PoseScore records of
// scorePoses), <dir>/best.bin (chosen as a float, then T_est [16], then the scores estimatePoseFromBest reports as n x 4 doubles) and the
// iterations per level to stdout.
#include <bpvo_hip/vo.hpp>

#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <string>

template <class T>
static std::vector<T> read_file(const std::string& path, size_t count)
{
  std::vector<T> v(count);
  std::ifstream f(path.c_str(), std::ios::binary);
  f.read(reinterpret_cast<char*>(v.data()), (std::streamsize) (count * sizeof(T)));
  if((size_t) f.gcount() != count * sizeof(T)) { std::fprintf(stderr, "short read: %s\n", path.c_str()); std::exit(3); }
  return v;
}

int main(int argc, char** argv)
{
  if(argc < 13) { std::fprintf(stderr, "arguments: see the head of this file\n"); return 2; }
  const std::string dir = argv[1];
  const int rows = std::atoi(argv[2]), cols = std::atoi(argv[3]);
  const bpvo::Matrix33 K = {{(float) std::atof(argv[4]), 0.0f, (float) std::atof(argv[6]), 0.0f, (float) std::atof(argv[5]), (float) std::atof(argv[7]), 0.0f, 0.0f, 1.0f}};
  const float baseline = (float) std::atof(argv[8]);
  const int n = std::atoi(argv[9]);
  const float tau = (float) std::atof(argv[10]);
  const int level = std::atoi(argv[11]);
  bpvo::AlgorithmParameters p;
  p.numPyramidLevels = 3;
  p.descriptor = std::string(argv[12]) == "bitplanes" ? BPVO_DESC_BITPLANES : BPVO_DESC_INTENSITY;
  p.lossFunction = BPVO_LOSS_TUKEY;
  p.verbosity = BPVO_VERB_SILENT;
  try {
    const size_t npix = (size_t) rows * cols;
    const std::vector<uint8_t> imgA = read_file<uint8_t>(dir + "/imgA.u8", npix), imgB = read_file<uint8_t>(dir + "/imgB.u8", npix);
    const std::vector<float> dispA = read_file<float>(dir + "/dispA.f32", npix), dispB = read_file<float>(dir + "/dispB.f32", npix);
    const std::vector<float> cand = read_file<float>(dir + "/candidates.f32", (size_t) n * 16);
    std::vector<bpvo::Matrix44> poses((size_t) n);
    for(int i = 0; i < n; ++i) std::memcpy(poses[(size_t) i].data(), &cand[16 * (size_t) i], 16 * sizeof(float));

    std::shared_ptr<bpvo::detail::Device> dev = std::make_shared<bpvo::detail::Device>(K, baseline, bpvo::ImageSize(rows, cols), p, 2, 1);
    bpvo::VisualOdometryFrame ref(dev, 0), cur(dev, 1);
    ref.setData(imgA.data(), dispA.data());
    ref.setTemplate();
    cur.setData(imgB.data(), dispB.data());
    bpvo::VisualOdometryPoseEstimator est(dev);

    const std::vector<bpvo::PoseScore> scores = est.scorePoses(&ref, &cur, level, poses, tau);
    std::ofstream(dir + "/scores.bin", std::ios::binary).write(reinterpret_cast<const char*>(scores.data()), (std::streamsize) (scores.size() * sizeof(bpvo::PoseScore)));

    bpvo::Matrix44 T_est;
    int chosen = -1;
    std::vector<bpvo::PoseScore> again;
    const std::vector<bpvo::OptimizerStatistics> stats = est.estimatePoseFromBest(&ref, &cur, poses, tau, T_est, &chosen, &again, level);
    std::ofstream f(dir + "/best.bin", std::ios::binary);
    const float chosen_f = (float) chosen;
    f.write(reinterpret_cast<const char*>(&chosen_f), sizeof(float));
    f.write(reinterpret_cast<const char*>(T_est.data()), 16 * sizeof(float));
    for(size_t i = 0; i < again.size(); ++i) {
      const double rec[4] = {again[i].cost_sum, again[i].score, (double) again[i].n_valid, (double) again[i].n_below};
      f.write(reinterpret_cast<const char*>(rec), sizeof(rec));
    }
    std::printf("iterations");
    for(size_t l = 0; l < stats.size(); ++l) std::printf(" %d", stats[l].numIterations);
    std::printf("\n");
  } catch(const std::exception& e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
  return 0;
}
