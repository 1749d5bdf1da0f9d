// The measurement-variance surface of include/bpvo_hip/vo.hpp, compiled by tests/test_disparity_variance_cpu.py (syntax only) and compiled and run
// by tests/test_gpu_disparity_variance.py:
//   disparity_variance_facade <dir> <rows> <cols> <fx> <fy> <cx> <cy> <baseline> <n_frames> <number_of_disparities>
//                             <measurement_sigma> <process_sigma> <gate> <max_fill_sigma> <radius> <noise_sigma> <min_sigma> <max_sigma>
// reads, per frame k, the rectified pair <dir>/left_k.u8 and <dir>/right_k.u8.  VisualOdometry with setDisparityFusion and setMeasurementVariance
// runs the pairs through block matching; VisualOdometrySequences with two sequences, both fusing, runs them too, sequence 1 alone with the
// variance on.  Writes <dir>/poses.bin ([n_frames][16] f32, the single path), <dir>/poses_seq.bin ([n_frames][2][16]), after the last frame
// <dir>/var.bin (the single path's map, then its fused disparity and variance) and <dir>/var_seq1.bin (sequence 1's), and prints per frame
// "invalid border flat floor ceiling model" of the single path.
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
static void write_maps(const std::string& path, const bpvo::MeasurementVarianceMap& v, const bpvo::FusedDisparity& m)
{
  std::ofstream f(path.c_str(), std::ios::binary);
  f.write(reinterpret_cast<const char*>(v.variance.data()), (std::streamsize) (v.variance.size() * sizeof(float)));
  f.write(reinterpret_cast<const char*>(m.disparity.data()), (std::streamsize) (m.disparity.size() * sizeof(float)));
  f.write(reinterpret_cast<const char*>(m.variance.data()), (std::streamsize) (m.variance.size() * sizeof(float)));
}

int main(int argc, char** argv)
{
  if(argc < 19) { std::fprintf(stderr, "arguments: see the head of this file\n"); return 2; }
  const std::string dir = argv[1];
  const int rows = std::atoi(argv[2]), cols = std::atoi(argv[3]);
  const bpvo::Matrix33 K = {{(float) std::atof(argv[4]), 0.0f, (float) std::atof(argv[6]), 0.0f, (float) std::atof(argv[5]), (float) std::atof(argv[7]), 0.0f, 0.0f, 1.0f}};
  const float baseline = (float) std::atof(argv[8]);
  const int n_frames = std::atoi(argv[9]);
  const bpvo::StereoParameters stereo(std::atoi(argv[10]));
  const bpvo::DisparityFusion fusion = bpvo::DisparityFusion::On((float) std::atof(argv[11]), (float) std::atof(argv[12]), (float) std::atof(argv[13]), (float) std::atof(argv[14]));
  const bpvo::MeasurementVariance variance = bpvo::MeasurementVariance::On(std::atoi(argv[15]), (float) std::atof(argv[16]), (float) std::atof(argv[17]), (float) std::atof(argv[18]));
  bpvo::AlgorithmParameters p;
  p.numPyramidLevels = 3;
  p.descriptor = BPVO_DESC_BITPLANES;
  p.lossFunction = BPVO_LOSS_HUBER;
  p.verbosity = BPVO_VERB_SILENT;
  const size_t npix = (size_t) rows * cols;
  try {
    bpvo::VisualOdometry vo(K, baseline, bpvo::ImageSize(rows, cols), p);
    vo.setDisparityFusion(fusion);
    vo.setMeasurementVariance(variance);
    bpvo::VisualOdometrySequences seqs(K, baseline, bpvo::ImageSize(rows, cols), 2, p);
    seqs.setDisparityFusion(fusion);
    seqs.setMeasurementVariance(bpvo::MeasurementVariance());      // (the context's setting: off)
    seqs.setMeasurementVariance(1, variance);
    bool refused = false;
    try { vo.setMeasurementVariance(bpvo::MeasurementVariance::On(8, 2.0f, 0.02f, 2.0f)); } catch(const bpvo::Error&) { refused = true; }
    if(!refused) { std::fprintf(stderr, "a radius of 8 was accepted\n"); return 1; }
    bool no_data = false;
    try { (void) vo.measurementVarianceInfo(); } catch(const bpvo::Error&) { no_data = true; }
    if(!no_data) { std::fprintf(stderr, "a record before the first stereo call\n"); return 1; }
    std::ofstream poses((dir + "/poses.bin").c_str(), std::ios::binary), poses_seq((dir + "/poses_seq.bin").c_str(), std::ios::binary);
    for(int k = 0; k < n_frames; ++k) {
      const std::vector<uint8_t> left = read_file<uint8_t>(dir + "/left_" + std::to_string(k) + ".u8", npix);
      const std::vector<uint8_t> right = read_file<uint8_t>(dir + "/right_" + std::to_string(k) + ".u8", npix);
      const bpvo::Result one = vo.addFrame(left.data(), right.data(), stereo);
      poses.write(reinterpret_cast<const char*>(one.pose.data()), 16 * sizeof(float));
      const bpvo::MeasurementVarianceInfo info = vo.measurementVarianceInfo();
      std::printf("%u %u %u %u %u %u\n", info.invalid, info.border, info.flat, info.floor, info.ceiling, info.model);
      std::vector<uint8_t> left2(left), right2(right);
      left2.insert(left2.end(), left.begin(), left.end());
      right2.insert(right2.end(), right.begin(), right.end());
      const std::vector<bpvo::Result> res = seqs.addFrames(left2.data(), right2.data(), stereo);
      for(int s = 0; s < 2; ++s) poses_seq.write(reinterpret_cast<const char*>(res[(size_t) s].pose.data()), 16 * sizeof(float));
    }
    write_maps(dir + "/var.bin", vo.measurementVariance(), vo.fusedDisparity());
    write_maps(dir + "/var_seq1.bin", seqs.measurementVariance(1), seqs.fusedDisparity(1));
    no_data = false;
    try { (void) seqs.measurementVariance(0); } catch(const bpvo::Error&) { no_data = true; }
    if(!no_data) { std::fprintf(stderr, "sequence 0 runs without the variance and has a map\n"); return 1; }
  } catch(const std::exception& e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
  return 0;
}
