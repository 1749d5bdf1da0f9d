// The disparity-fusion surface of include/bpvo_hip/vo.hpp, compiled by tests/test_disparity_fusion_cpu.py (syntax only) and compiled and run by
// tests/test_gpu_disparity_fusion.py:
//   disparity_fusion_facade <dir> <rows> <cols> <fx> <fy> <cx> <cy> <baseline> <n_frames> <measurement_sigma> <process_sigma> <gate> <max_fill_sigma>
// reads, per frame k, <dir>/img_k.u8 and <dir>/disp_k.f32.  VisualOdometry with setDisparityFusion runs the frames; VisualOdometrySequences with
// two sequences runs them too, sequence 1 alone in mode 1.  Writes <dir>/poses.bin ([n_frames][16] f32, the single path), <dir>/poses_seq.bin
// ([n_frames][2][16]), after the last frame <dir>/fused.bin (disparity then variance of the single path) and <dir>/fused_seq1.bin (sequence 1's),
// and prints per frame "fused replaced measured filled none predicted" of the single path.
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
static void write_maps(const std::string& path, const bpvo::FusedDisparity& m)
{
  std::ofstream f(path.c_str(), std::ios::binary);
  f.write(reinterpret_cast<const char*>(m.disparity.data()), (std::streamsize) (m.disparity.size() * sizeof(float)));
  f.write(reinterpret_cast<const char*>(m.variance.data()), (std::streamsize) (m.variance.size() * sizeof(float)));
}

int main(int argc, char** argv)
{
  if(argc < 14) { std::fprintf(stderr, "arguments: see the head of this file\n"); return 2; }
  const std::string dir = argv[1];
  const int rows = std::atoi(argv[2]), cols = std::atoi(argv[3]);
  const bpvo::Matrix33 K = {{(float) std::atof(argv[4]), 0.0f, (float) std::atof(argv[6]), 0.0f, (float) std::atof(argv[5]), (float) std::atof(argv[7]), 0.0f, 0.0f, 1.0f}};
  const float baseline = (float) std::atof(argv[8]);
  const int n_frames = std::atoi(argv[9]);
  const bpvo::DisparityFusion fusion = bpvo::DisparityFusion::On((float) std::atof(argv[10]), (float) std::atof(argv[11]), (float) std::atof(argv[12]), (float) std::atof(argv[13]));
  bpvo::AlgorithmParameters p;
  p.numPyramidLevels = 3;
  p.descriptor = BPVO_DESC_BITPLANES;
  p.lossFunction = BPVO_LOSS_HUBER;
  p.verbosity = BPVO_VERB_SILENT;
  const size_t npix = (size_t) rows * cols;
  try {
    bpvo::VisualOdometry vo(K, baseline, bpvo::ImageSize(rows, cols), p);
    vo.setDisparityFusion(fusion);
    bpvo::VisualOdometrySequences seqs(K, baseline, bpvo::ImageSize(rows, cols), 2, p);
    seqs.setDisparityFusion(bpvo::DisparityFusion());      // (the context's setting: off)
    seqs.setDisparityFusion(1, fusion);
    bool refused = false;
    try { vo.setDisparityFusion(bpvo::DisparityFusion::On(0.0f, 0.0f, 3.0f, 0.0f)); } catch(const bpvo::Error&) { refused = true; }
    if(!refused) { std::fprintf(stderr, "a measurement_sigma of 0 was accepted\n"); return 1; }
    std::ofstream poses((dir + "/poses.bin").c_str(), std::ios::binary), poses_seq((dir + "/poses_seq.bin").c_str(), std::ios::binary);
    for(int k = 0; k < n_frames; ++k) {
      const std::vector<uint8_t> img = read_file<uint8_t>(dir + "/img_" + std::to_string(k) + ".u8", npix);
      const std::vector<float> disp = read_file<float>(dir + "/disp_" + std::to_string(k) + ".f32", npix);
      const bpvo::Result one = vo.addFrame(img.data(), disp.data());
      poses.write(reinterpret_cast<const char*>(one.pose.data()), 16 * sizeof(float));
      const bpvo::DisparityFusionInfo info = vo.disparityFusionInfo();
      std::printf("%u %u %u %u %u %d\n", info.fused, info.replaced, info.measured, info.filled, info.none, info.predicted);
      std::vector<uint8_t> img2(img);
      img2.insert(img2.end(), img.begin(), img.end());
      std::vector<float> disp2(disp);
      disp2.insert(disp2.end(), disp.begin(), disp.end());
      const std::vector<bpvo::Result> res = seqs.addFrames(img2.data(), disp2.data());
      for(int s = 0; s < 2; ++s) poses_seq.write(reinterpret_cast<const char*>(res[(size_t) s].pose.data()), 16 * sizeof(float));
    }
    write_maps(dir + "/fused.bin", vo.fusedDisparity());
    write_maps(dir + "/fused_seq1.bin", seqs.fusedDisparity(1));
    if(seqs.disparityFusionInfo(0).measured != 0) { std::fprintf(stderr, "sequence 0 runs in mode 0 and fused\n"); return 1; }
  } catch(const std::exception& e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
  return 0;
}
