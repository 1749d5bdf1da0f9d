// The motion-stereo surface of include/bpvo_hip/vo.hpp, compiled by tests/test_motion_stereo_cpu.py (syntax only) and compiled and run by
// tests/test_gpu_motion_stereo.py:
//   motion_stereo_facade <dir> <rows> <cols> <fx> <fy> <cx> <cy> <baseline> <n_frames>
//                        <measurement_sigma> <process_sigma> <gate> <max_fill_sigma> <radius> <steps> <min_gain> <noise_sigma> <min_sigma> <max_sigma> <ms_gate>
// reads, per frame k, <dir>/img_k.u8 and <dir>/disp_k.f32.  VisualOdometry with setDisparityFusion and setMotionStereo runs the frames;
// VisualOdometrySequences with two sequences, both fusing, runs them too, sequence 1 alone with motion stereo on.  The settings are read back
// and must round-trip.  Writes <dir>/poses.bin ([n_frames][16] f32, the single path) and <dir>/poses_seq.bin ([n_frames][2][16]), and prints per
// frame "no_prior low_parallax border edge flat rejected fused launched" of the single path.
#include <bpvo_hip/vo.hpp>

#include <cstdio>
#include <cstdlib>
#include <cstring>
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
static bool same(const bpvo_hip_motion_stereo& a, const bpvo_hip_motion_stereo& b) { return std::memcmp(&a, &b, sizeof(a)) == 0; }

int main(int argc, char** argv)
{
  if(argc < 21) { std::fprintf(stderr, "arguments: see the head of this file\n"); return 2; }
  const std::string dir = argv[1];
  const int rows = std::atoi(argv[2]), cols = std::atoi(argv[3]);
  const bpvo::Matrix33 K = {{(float) std::atof(argv[4]), 0.0f, (float) std::atof(argv[6]), 0.0f, (float) std::atof(argv[5]), (float) std::atof(argv[7]), 0.0f, 0.0f, 1.0f}};
  const float baseline = (float) std::atof(argv[8]);
  const int n_frames = std::atoi(argv[9]);
  const bpvo::DisparityFusion fusion = bpvo::DisparityFusion::On((float) std::atof(argv[10]), (float) std::atof(argv[11]), (float) std::atof(argv[12]), (float) std::atof(argv[13]));
  const bpvo::MotionStereo ms = bpvo::MotionStereo::On(std::atoi(argv[14]), std::atoi(argv[15]), (float) std::atof(argv[16]), (float) std::atof(argv[17]),
                                                       (float) std::atof(argv[18]), (float) std::atof(argv[19]), (float) std::atof(argv[20]));
  bpvo::AlgorithmParameters p;
  p.numPyramidLevels = 2;
  p.descriptor = BPVO_DESC_BITPLANES;
  p.lossFunction = BPVO_LOSS_HUBER;
  p.verbosity = BPVO_VERB_SILENT;
  const size_t npix = (size_t) rows * cols;
  try {
    bpvo::VisualOdometry vo(K, baseline, bpvo::ImageSize(rows, cols), p);
    vo.setDisparityFusion(fusion);
    if(vo.motionStereo().mode != 0) { std::fprintf(stderr, "on before it was set\n"); return 1; }
    vo.setMotionStereo(ms);
    if(!same(vo.motionStereo(), ms)) { std::fprintf(stderr, "the setting did not round-trip\n"); return 1; }
    bpvo::VisualOdometrySequences seqs(K, baseline, bpvo::ImageSize(rows, cols), 2, p);
    seqs.setDisparityFusion(fusion);
    seqs.setMotionStereo(bpvo::MotionStereo());      // (the context's setting: off)
    seqs.setMotionStereo(1, ms);
    if(!same(seqs.motionStereo(1), ms) || seqs.motionStereo(0).mode != 0) { std::fprintf(stderr, "a sequence's setting did not round-trip\n"); return 1; }
    bool refused = false;
    try { vo.setMotionStereo(bpvo::MotionStereo::On(4, 2, 0.25f, 2.0f, 0.02f, 2.0f, 3.0f)); } catch(const bpvo::Error&) { refused = true; }
    if(!refused || !same(vo.motionStereo(), ms)) { std::fprintf(stderr, "a radius of 4 was accepted, or changed the setting\n"); return 1; }
    std::ofstream poses((dir + "/poses.bin").c_str(), std::ios::binary), poses_seq((dir + "/poses_seq.bin").c_str(), std::ios::binary);
    for(int k = 0; k < n_frames; ++k) {
      const std::vector<uint8_t> img = read_file<uint8_t>(dir + "/img_" + std::to_string(k) + ".u8", npix);
      const std::vector<float> disp = read_file<float>(dir + "/disp_" + std::to_string(k) + ".f32", npix);
      const bpvo::Result one = vo.addFrame(img.data(), disp.data());
      poses.write(reinterpret_cast<const char*>(one.pose.data()), 16 * sizeof(float));
      const bpvo::MotionStereoInfo info = vo.motionStereoInfo();
      std::printf("%u %u %u %u %u %u %u %d\n", info.no_prior, info.low_parallax, info.border, info.edge, info.flat, info.rejected, info.fused, info.launched);
      std::vector<uint8_t> img2(img);
      img2.insert(img2.end(), img.begin(), img.end());
      std::vector<float> disp2(disp);
      disp2.insert(disp2.end(), disp.begin(), disp.end());
      const std::vector<bpvo::Result> res = seqs.addFrames(img2.data(), disp2.data());
      for(int s = 0; s < 2; ++s) poses_seq.write(reinterpret_cast<const char*>(res[(size_t) s].pose.data()), 16 * sizeof(float));
      if(seqs.motionStereoInfo(0).launched != 0 || seqs.motionStereoInfo(1).launched != (k > 0 ? 1 : 0)) { std::fprintf(stderr, "frame %d: launches\n", k); return 1; }
    }
  } catch(const std::exception& e) {
    std::fprintf(stderr, "error: %s\n", e.what());
    return 1;
  }
  return 0;
}
