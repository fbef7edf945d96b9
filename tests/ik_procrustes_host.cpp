// Host restatement of K36's Procrustes step for tests/test_ik.py: p2c_procrustes::solve (csrc/p2c_procrustes_dev.h, host-callable)
// on 3x3 matrices read as raw doubles. usage: ik_procrustes_host IN OUT -- IN holds n * 9 doubles (H, row-major), OUT gets n * 9
// doubles (R, row-major).
#include <cmath>
#include <cstdio>
#include <vector>

using std::copysign;
using std::sqrt;

#include "p2c_procrustes_dev.h"

int main(int argc, char **argv) {
  if (argc != 3) return 2;
  std::FILE *in = std::fopen(argv[1], "rb");
  if (!in) return 3;
  std::vector<double> data;
  double buf[9];
  while (std::fread(buf, sizeof(double), 9, in) == 9) data.insert(data.end(), buf, buf + 9);
  std::fclose(in);
  std::FILE *out = std::fopen(argv[2], "wb");
  if (!out) return 4;
  for (size_t n = 0; n + 9 <= data.size(); n += 9) {
    double H[3][3], R[3][3], sum;
    for (int i = 0; i < 9; ++i) H[i / 3][i % 3] = data[n + i];
    p2c_procrustes::solve(H, R, sum);
    for (int i = 0; i < 9; ++i) buf[i] = R[i / 3][i % 3];
    if (std::fwrite(buf, sizeof(double), 9, out) != 9) return 5;
  }
  return std::fclose(out) == 0 ? 0 : 6;
}
