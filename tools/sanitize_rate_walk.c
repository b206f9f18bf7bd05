/*
 * tools/sanitize_rate_walk.c -- stand-alone driver of oracle/wrapper_oracle.c for tools/sanitize_host.sh: one processor through a host that
 * changes its rate in mid-life (wo_set_sample_rate: up, down, the same rate, a restart at the same rate, odd block lengths, gains ramping
 * across every change), built together with the oracle under the sanitizers and run as a program of its own.  Exit status 0: the walk ran
 * and kept the contract of processor_core_2.cc:421-429 -- a new rate empties the FIFO (a leg's first 9 ms are zeros), the same rate does not.
 */
#include <math.h>
#include <stdio.h>
#include <stdlib.h>

typedef void (*wo_hop_fn)(const float* in160, float* out240, void* user);
typedef struct WoProcessor WoProcessor;
WoProcessor* wo_create(double sample_rate, wo_hop_fn hop, void* user);
void wo_destroy(WoProcessor* p);
void wo_set_sample_rate(WoProcessor* p, double sample_rate);
void wo_set_input_gain(WoProcessor* p, double db);
void wo_set_output_gain(WoProcessor* p, double db);
int wo_process(WoProcessor* p, const float* in, float* out, int n);
int wo_fifo_fill(const WoProcessor* p);
void wo_gain_state(const WoProcessor* p, double* in_target, double* in_now, double* out_target, double* out_now);

static void hop(const float* in160, float* out240, void* user) {
  ++*(int*)user;
  for (int i = 0; i < 240; ++i) out240[i] = in160[(2 * i) / 3];
}

int main(void) {
  static const struct { double rate; int block, n, restarts; double gin, gout; } legs[] = {
      {44100, 441, 3000, 1, -6, 3},  {48000, 480, 1500, 1, -46, -40}, {44100, 64, 2000, 1, 0, 6},   {44100, 441, 1500, 0, -40, -36},
      {16000, 333, 1200, 1, 3, 0},   {192000, 4001, 9000, 1, -40, 0}, {8000, 1, 300, 1, 0, 0},      {8000.5, 97, 900, 1, 0, -50},
      {96000, 960, 4000, 1, 0, 0},   {22050, 1024, 2500, 1, 6, 6},    {22050, 1, 700, 0, 0, 0}};
  int hops = 0, bad = 0;
  WoProcessor* p = wo_create(legs[0].rate, hop, &hops);
  for (unsigned l = 0; l < sizeof(legs) / sizeof(legs[0]); ++l) {
    if (l) wo_set_sample_rate(p, legs[l].rate);
    wo_set_input_gain(p, legs[l].gin);
    wo_set_output_gain(p, legs[l].gout);
    float* x = (float*)malloc(sizeof(float) * (size_t)legs[l].n);
    float* y = (float*)malloc(sizeof(float) * (size_t)legs[l].n);
    for (int i = 0; i < legs[l].n; ++i) x[i] = 0.4f * (float)sin(0.05 * i + l) + 0.1f;
    for (int at = 0; at < legs[l].n; at += legs[l].block) {
      const int m = legs[l].n - at < legs[l].block ? legs[l].n - at : legs[l].block;
      if (wo_process(p, x + at, y + at, m) != 0) ++bad;
    }
    const int head = (int)(0.009 * legs[l].rate);
    int zeros = 1;
    for (int i = 0; i < head; ++i) zeros = zeros && y[i] == 0.0f;
    for (int i = 0; i < legs[l].n; ++i) if (!isfinite(y[i])) ++bad;
    if (zeros != legs[l].restarts) { fprintf(stderr, "leg %u: restarted %d, expected %d\n", l, zeros, legs[l].restarts); ++bad; }
    double a, b, c, d;
    wo_gain_state(p, &a, &b, &c, &d);
    if (a != legs[l].gin || c != legs[l].gout || wo_fifo_fill(p) < 0 || wo_fifo_fill(p) >= 480) ++bad;
    free(x); free(y);
  }
  /* the restart at the present rate, and a rate the chain cannot take followed by one it can */
  wo_set_sample_rate(p, 8000.0); wo_set_sample_rate(p, 22050.0);
  if (wo_fifo_fill(p) != 0) ++bad;
  wo_set_sample_rate(p, 0.0);
  float z[64] = {0}, o[64];
  if (wo_process(p, z, o, 64) == 0) ++bad;   /* not ready: zeros and the reference's error code */
  wo_set_sample_rate(p, 48000.0);
  if (wo_process(p, z, o, 64) != 0) ++bad;
  wo_destroy(p);
  printf("rate walk: %d hops, %d complaints\n", hops, bad);
  return bad ? 1 : 0;
}
