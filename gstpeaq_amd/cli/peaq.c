/* peaq.c -- the `peaq REFFILE TESTFILE` command-line tool on the MI355X engine.
 *
 * Same interface as the reference's CLI (src/peaq.c): options --basic (default),
 * --advanced, --version; prints
 *     Objective Difference Grade: %.3f
 *     Distortion Index: %.3f
 * (peaq.c:217-220); exit status 0, 1 on usage errors (:110-133), 2 when the
 * engine cannot be set up (:147-195).  The reference builds a GStreamer pipeline
 * filesrc ! wavparse ! audioconvert ! audioresample ! peaq (:154-209); this tool
 * reads RIFF/WAVE itself (PCM 8/16/24/32 bit and IEEE float 32/64, mono or
 * stereo) and feeds the engine's session API directly, so that it works on a
 * box without gst-plugins-good.  Integer PCM is scaled by 1/2^(bits-1) like
 * audioconvert does (S16 -> x/32768, verified in SURVEY.md 8(c)).  The ear
 * models are defined for 48 kHz only (earmodel.c:43): files at another rate are
 * converted first, as the reference's `audioresample` does -- here with a
 * Kaiser-windowed sinc interpolator whose parameters are the measured ones of
 * that `audioresample` (resample_to_48k below).  Against the real reference
 * chain ODG/DI agree to 6e-5 in seven of eight pinned cases and 2.3e-3 in the
 * eighth (tests/test_cli_resampler.py; stated tolerance 5e-3).  48 kHz files:
 * digit for digit in both versions -- the advanced version's filter bank runs
 * in FP64 like the reference (the engine's default); PEAQ_AMD_FIR=f16x3 selects
 * the reduced-precision bank (held to 1e-6 in ODG/DI, include/peaq_amd.h).
 * --no-resample refuses files at other rates instead.
 * --device-resample hands files at another rate to the engine as they are (peaq_run_pair_rate): the same converter
 * as a kernel, for both files at once; rates the device does not take, two files at different rates, and the modes
 * that work on 48 kHz samples in host memory (--interval, PEAQ_AMD_CLI_STREAM, PEAQ_AMD_CLI_DUMP) still go through
 * resample_to_48k, with a note on stderr.
 * --interval=SECONDS also prints, before those two lines, one line per reading taken every SECONDS of the (resampled)
 * signals, "Time %.3f s: ODG %.3f, DI %.3f" -- what the element's odg / di properties read at that point of the stream
 * (gstpeaq.c:484-497; peaq_run_pair_trajectory).
 * --windows=SECONDS[:HOP_SECONDS] (basic version) also prints, before those two lines, one line per window of SECONDS
 * taken every HOP_SECONDS through the signals as scored, "window START_S END_S FRAMES ODG DI": the reading of the
 * frames the window covers, in the context of the running stream (peaq_run_pair_windows).
 * --advanced --spans=SECONDS[:HOP_SECONDS] is the same for the advanced version, "span START_S END_S FRAMES BLOCKS ODG
 * DI": the reading of the FFT frames and filter-bank blocks the span covers (peaq_run_pair_adv_spans).
 * --list=FILE scores many pairs in one run: FILE holds one pair per line, REF<TAB>TEST (empty lines and lines that
 * start with # are skipped).  The files' data chunks are handed to the engine as they are, in their own sample format
 * (peaq_batch_run_host: decoded, converted to 48 kHz and, with --align, aligned on the device), grouped by format,
 * channel count and rate; one line per pair in list order, REF<TAB>TEST<TAB>ODG<TAB>DI.  Nothing is scored (exit
 * status 2) if a file cannot be read, the two files of a pair differ in format, or a rate is one the device converter
 * does not take.  Within such a group a reference path that several lines name (compared as the exact string) is read once
 * and uploaded once per chunk, the lines ordered by reference for the call and printed in list order all the same
 * (peaq_batch_run_host_refs); --no-share-refs reads every line's reference again and hands plain pairs to
 * peaq_batch_run_host.  Behind the results one line on stderr says how many references were read for how many pairs.
 */
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "peaq_amd.h"

typedef struct
{
  float *samples;               /* interleaved */
  size_t frames;                /* samples per channel */
  int channels, rate;
} wav_t;

static uint32_t
rd32 (const unsigned char *p)
{
  return (uint32_t) p[0] | ((uint32_t) p[1] << 8) | ((uint32_t) p[2] << 16) | ((uint32_t) p[3] << 24);
}

static int
wav_read (const char *path, wav_t * w)
{
  FILE *f = fopen (path, "rb");
  unsigned char hdr[12], ck[8];
  int fmt_tag = 0, bits = 0, have_fmt = 0, block_align = 0;
  memset (w, 0, sizeof *w);
  if (!f) {
    fprintf (stderr, "Error: cannot open %s\n", path);
    return -1;
  }
  if (fread (hdr, 1, 12, f) != 12 || memcmp (hdr, "RIFF", 4) || memcmp (hdr + 8, "WAVE", 4)) {
    fprintf (stderr, "Error: %s is not a RIFF/WAVE file\n", path);
    fclose (f);
    return -1;
  }
  while (fread (ck, 1, 8, f) == 8) {
    uint32_t size = rd32 (ck + 4);
    if (!memcmp (ck, "fmt ", 4)) {
      unsigned char fmt[40];
      uint32_t n = size < sizeof fmt ? size : sizeof fmt;
      if (size < 16 || fread (fmt, 1, n, f) != n)
        break;
      fmt_tag = fmt[0] | (fmt[1] << 8);
      w->channels = fmt[2] | (fmt[3] << 8);
      w->rate = (int) rd32 (fmt + 4);
      block_align = fmt[12] | (fmt[13] << 8);
      bits = fmt[14] | (fmt[15] << 8);
      if (fmt_tag == 0xFFFE && size >= 26)      /* WAVE_FORMAT_EXTENSIBLE: sub-format GUID */
        fmt_tag = fmt[24] | (fmt[25] << 8);
      have_fmt = 1;
      if (size > n)
        fseek (f, (long) (size - n), SEEK_CUR);
      if (size & 1)
        fseek (f, 1, SEEK_CUR);
    } else if (!memcmp (ck, "data", 4) && have_fmt) {
      size_t bytes_per = (size_t) bits / 8, total, i;
      unsigned char *raw;
      if (w->channels < 1 || w->channels > 2 || block_align != (int) bytes_per * w->channels ||
          !((fmt_tag == 1 && (bits == 8 || bits == 16 || bits == 24 || bits == 32)) ||
              (fmt_tag == 3 && (bits == 32 || bits == 64)))) {
        fprintf (stderr, "Error: %s: unsupported WAVE format (tag %d, %d bit, %d channels)\n", path,
            fmt_tag, bits, w->channels);
        fclose (f);
        return -1;
      }
      raw = malloc (size ? size : 1);
      total = fread (raw, 1, size, f) / bytes_per;     /* tolerate a truncated data chunk */
      total -= total % w->channels;
      w->frames = total / w->channels;
      w->samples = malloc ((total ? total : 1) * sizeof (float));
      for (i = 0; i < total; i++) {
        const unsigned char *p = raw + i * bytes_per;
        double v;
        if (fmt_tag == 3) {
          if (bits == 32) {
            float t;
            memcpy (&t, p, 4);
            v = t;
          } else {
            memcpy (&v, p, 8);
          }
        } else if (bits == 8) {
          v = ((int) p[0] - 128) / 128.;
        } else if (bits == 16) {
          v = (int16_t) (p[0] | (p[1] << 8)) / 32768.;
        } else if (bits == 24) {
          int32_t t = (int32_t) ((uint32_t) p[0] << 8 | (uint32_t) p[1] << 16 | (uint32_t) p[2] << 24) >> 8;
          v = t / 8388608.;
        } else {
          v = (int32_t) rd32 (p) / 2147483648.;
        }
        w->samples[i] = (float) v;
      }
      free (raw);
      fclose (f);
      return 0;
    } else {
      fseek (f, (long) (size + (size & 1)), SEEK_CUR);
    }
  }
  fprintf (stderr, "Error: %s: no usable fmt/data chunks\n", path);
  fclose (f);
  return -1;
}

/* ---- --list: the data chunk as it is, for peaq_batch_run_host ---- */
typedef struct
{
  unsigned char *bytes;         /* the data chunk, whole samples per channel only */
  size_t frames;                /* samples per channel */
  int format;                   /* PEAQ_PCM_* */
  int channels, rate;
} raw_t;

static int
wav_read_raw (const char *path, raw_t * w)
{
  FILE *f = fopen (path, "rb");
  unsigned char hdr[12], ck[8];
  int fmt_tag = 0, bits = 0, have_fmt = 0, block_align = 0;
  memset (w, 0, sizeof *w);
  if (!f) {
    fprintf (stderr, "Error: cannot open %s\n", path);
    return -1;
  }
  if (fread (hdr, 1, 12, f) != 12 || memcmp (hdr, "RIFF", 4) || memcmp (hdr + 8, "WAVE", 4)) {
    fprintf (stderr, "Error: %s is not a RIFF/WAVE file\n", path);
    fclose (f);
    return -1;
  }
  while (fread (ck, 1, 8, f) == 8) {
    uint32_t size = rd32 (ck + 4);
    if (!memcmp (ck, "fmt ", 4)) {
      unsigned char fmt[40];
      uint32_t n = size < sizeof fmt ? size : sizeof fmt;
      if (size < 16 || fread (fmt, 1, n, f) != n)
        break;
      fmt_tag = fmt[0] | (fmt[1] << 8);
      w->channels = fmt[2] | (fmt[3] << 8);
      w->rate = (int) rd32 (fmt + 4);
      block_align = fmt[12] | (fmt[13] << 8);
      bits = fmt[14] | (fmt[15] << 8);
      if (fmt_tag == 0xFFFE && size >= 26)
        fmt_tag = fmt[24] | (fmt[25] << 8);
      have_fmt = 1;
      if (size > n)
        fseek (f, (long) (size - n), SEEK_CUR);
      if (size & 1)
        fseek (f, 1, SEEK_CUR);
    } else if (!memcmp (ck, "data", 4) && have_fmt) {
      size_t bytes_per = (size_t) bits / 8, total;
      w->format = fmt_tag == 3 ? (bits == 32 ? PEAQ_PCM_F32 : bits == 64 ? PEAQ_PCM_F64 : -1)
          : fmt_tag == 1 ? (bits == 8 ? PEAQ_PCM_U8 : bits == 16 ? PEAQ_PCM_S16 : bits == 24 ? PEAQ_PCM_S24 : bits ==
          32 ? PEAQ_PCM_S32 : -1) : -1;
      if (w->channels < 1 || w->channels > 2 || block_align != (int) bytes_per * w->channels || w->format < 0) {
        fprintf (stderr, "Error: %s: unsupported WAVE format (tag %d, %d bit, %d channels)\n", path,
            fmt_tag, bits, w->channels);
        fclose (f);
        return -1;
      }
      w->bytes = malloc (size ? size : 1);
      total = fread (w->bytes, 1, size, f) / bytes_per;        /* tolerate a truncated data chunk */
      w->frames = total / w->channels;
      fclose (f);
      return 0;
    } else {
      fseek (f, (long) (size + (size & 1)), SEEK_CUR);
    }
  }
  fprintf (stderr, "Error: %s: no usable fmt/data chunks\n", path);
  fclose (f);
  return -1;
}

/* --list with shared references: an order of the lines by a key and, among equal keys, by line */
static char **sort_names;       /* [2 * line]: the reference's path */
static const size_t *sort_key;  /* [line] */

static int
by_ref_name (const void *a, const void *b)
{
  const size_t x = *(const size_t *) a, y = *(const size_t *) b;
  const int c = strcmp (sort_names[2 * x], sort_names[2 * y]);
  return c ? c : (x > y) - (x < y);
}

static int
by_key (const void *a, const void *b)
{
  const size_t x = *(const size_t *) a, y = *(const size_t *) b;
  return sort_key[x] != sort_key[y] ? (sort_key[x] > sort_key[y]) - (sort_key[x] < sort_key[y]) : (x > y) - (x < y);
}

/* --match-gain: the record as text, in the style of the delay line: per channel the gain applied in dB, "inverted" for
 * a negative factor, and the flags of a channel left unmatched by name */
static void
format_gain (char *buf, size_t size, const peaq_gain * g, int channels)
{
  static const char *const names[4] = { "silent", "nonfinite", "zero", "range" };
  size_t used = 0;
  int c, b;
  buf[0] = 0;
  for (c = 0; c < channels && used < size; c++) {
    used += (size_t) snprintf (buf + used, size - used, "%s%+.2f dB%s", c ? ", " : "", 20. * log10 (fabs (g->gain[c])),
        g->gain[c] < 0. ? " inverted" : "");
    for (b = 0; b < 4 && used < size; b++)
      if (g->flags[c] & (1u << b))
        used += (size_t) snprintf (buf + used, size - used, " [%s]", names[b]);
  }
}

/* scores the pairs of `list_path`; the exit status */
static int
run_list (const char *list_path, int advanced, double level, uint32_t align_lag, int share_refs, int gain_mode,
    double max_gain_db)
{
  FILE *f = fopen (list_path, "r");
  char *line = NULL, **names = NULL;
  size_t cap = 0, n_pairs = 0, room = 0, p, q;
  raw_t *raw = NULL;
  peaq_result *res = NULL;
  peaq_gain *gains = NULL;
  peaq_host_pair *hp = NULL;
  size_t *members = NULL;
  char *done = NULL;
  size_t *first = NULL;         /* [line]: the first line that names the same reference path (share_refs) */
  size_t n_read = 0;
  peaq_host_signal *hs = NULL;
  peaq_host_test *ht = NULL;
  peaq_ctx *ctx = NULL;
  ssize_t len;
  if (!f) {
    fprintf (stderr, "Error: cannot open %s\n", list_path);
    return 2;
  }
  while ((len = getline (&line, &cap, f)) >= 0) {
    char *tab;
    while (len > 0 && (line[len - 1] == '\n' || line[len - 1] == '\r'))
      line[--len] = 0;
    if (!len || line[0] == '#')
      continue;
    tab = strchr (line, '\t');
    if (!tab || !tab[1] || tab == line || strchr (tab + 1, '\t')) {
      fprintf (stderr, "Error: %s: a line is not REF<TAB>TEST: %s\n", list_path, line);
      return 2;
    }
    if (n_pairs == room) {
      room = room ? 2 * room : 64;
      names = realloc (names, 2 * room * sizeof *names);
    }
    *tab = 0;
    names[2 * n_pairs] = strdup (line);
    names[2 * n_pairs + 1] = strdup (tab + 1);
    n_pairs++;
  }
  free (line);
  fclose (f);
  raw = calloc (2 * n_pairs + 1, sizeof *raw);
  res = calloc (n_pairs + 1, sizeof *res);
  gains = calloc (n_pairs + 1, sizeof *gains);
  hp = calloc (n_pairs + 1, sizeof *hp);
  members = calloc (n_pairs + 1, sizeof *members);
  done = calloc (n_pairs + 1, 1);
  first = calloc (n_pairs + 1, sizeof *first);
  hs = calloc (n_pairs + 1, sizeof *hs);
  ht = calloc (n_pairs + 1, sizeof *ht);
  for (p = 0; p < n_pairs; p++)
    first[p] = p;
  if (share_refs) {
    for (p = 0; p < n_pairs; p++)
      members[p] = p;
    sort_names = names;
    qsort (members, n_pairs, sizeof *members, by_ref_name);
    for (p = 1; p < n_pairs; p++)
      if (!strcmp (names[2 * members[p]], names[2 * members[p - 1]]))
        first[members[p]] = first[members[p - 1]];
  }
  for (p = 0; p < n_pairs; p++) {
    const raw_t *r = &raw[2 * p], *t = &raw[2 * p + 1];
    if (first[p] != p)
      raw[2 * p] = raw[2 * first[p]];   /* (the same bytes: nothing is freed before the process ends) */
    else if (wav_read_raw (names[2 * p], &raw[2 * p]))
      return 2;
    else
      n_read++;
    if (wav_read_raw (names[2 * p + 1], &raw[2 * p + 1]))
      return 2;
    if (r->format != t->format || r->channels != t->channels || r->rate != t->rate) {
      fprintf (stderr, "Error: %s and %s differ in sample format, channel count or rate\n", names[2 * p], names[2 * p + 1]);
      return 2;
    }
    if (r->rate != 48000 && !peaq_resample_supported ((uint32_t) r->rate)) {
      fprintf (stderr, "Note: the device converter does not take %d Hz (%s)\n", r->rate, names[2 * p]);
      return 2;
    }
  }
  if (n_pairs && peaq_ctx_create (getenv ("PEAQ_AMD_DEVICE") ? atoi (getenv ("PEAQ_AMD_DEVICE")) : 0, &ctx) != PEAQ_OK) {
    printf ("Error: peaq engine could not be instantiated - %s\n", peaq_last_error ());
    return 2;
  }
  for (p = 0; p < n_pairs; p++) {
    /* the pairs that share this one's format, channel count and rate: one call */
    peaq_feed feed;
    size_t n = 0;
    if (done[p])
      continue;
    for (q = p; q < n_pairs; q++)
      if (!done[q] && raw[2 * q].format == raw[2 * p].format && raw[2 * q].channels == raw[2 * p].channels
          && raw[2 * q].rate == raw[2 * p].rate) {
        members[n++] = q;
        done[q] = 1;
      }
    if (share_refs) {           /* the group's lines by reference, a reference's lines in list order */
      sort_key = first;
      qsort (members, n, sizeof *members, by_key);
    }
    for (q = 0; q < n; q++) {
      hp[q].ref = raw[2 * members[q]].bytes;
      hp[q].test = raw[2 * members[q] + 1].bytes;
      hp[q].n_ref = raw[2 * members[q]].frames;
      hp[q].n_test = raw[2 * members[q] + 1].frames;
    }
    memset (&feed, 0, sizeof feed);
    feed.struct_size = (uint32_t) sizeof feed;
    feed.format = raw[2 * p].format;
    feed.channels = raw[2 * p].channels;
    feed.rate = (uint32_t) raw[2 * p].rate;
    feed.align_max_lag = align_lag;
    {
      peaq_result *out = malloc (n * sizeof *out);
      peaq_gain *gout = malloc ((n + 1) * sizeof *gout);
      size_t n_refs = 0;
      for (q = 0; (share_refs || gain_mode) && q < n; q++) {   /* (matched pairs not shared: one test per reference) */
        if (!q || !share_refs || first[members[q]] != first[members[q - 1]]) {
          hs[n_refs].data = hp[q].ref;
          hs[n_refs++].n = hp[q].n_ref;
        }
        ht[q].data = hp[q].test;
        ht[q].n = hp[q].n_test;
        ht[q].ref = (uint32_t) (n_refs - 1);
      }
      if ((gain_mode ? peaq_batch_run_host_matched (ctx, advanced, level, &feed, gain_mode, max_gain_db, n_refs, hs, n, ht,
                  out, NULL, gout)
              : share_refs ? peaq_batch_run_host_refs (ctx, advanced, level, &feed, n_refs, hs, n, ht, out, NULL)
              : peaq_batch_run_host (ctx, advanced, level, &feed, n, hp, out, NULL)) != PEAQ_OK) {
        fprintf (stderr, "Error: %s\n", peaq_last_error ());
        return 2;
      }
      for (q = 0; q < n; q++) {
        res[members[q]] = out[q];
        if (gain_mode)
          gains[members[q]] = gout[q];
      }
      free (out);
      free (gout);
    }
  }
  for (p = 0; p < n_pairs; p++) {
    if (gain_mode) {
      char text[256];
      format_gain (text, sizeof text, &gains[p], raw[2 * p].channels);
      printf ("%s\t%s\t%.3f\t%.3f\tGain: %s\n", names[2 * p], names[2 * p + 1], res[p].odg, res[p].di, text);
    } else
      printf ("%s\t%s\t%.3f\t%.3f\n", names[2 * p], names[2 * p + 1], res[p].odg, res[p].di);
  }
  fflush (stdout);
  fprintf (stderr, "Note: %zu %s read for %zu pairs\n", n_read, share_refs ? "distinct references" : "references", n_pairs);
  if (ctx)
    peaq_ctx_destroy (ctx);
  return 0;
}

/* ---- sample-rate conversion to 48 kHz (stands in for audioresample, peaq.c:154-209) ----
 * y[m] = sum_n x[n] h(t_m - n), t_m = m rate / 48000 - 1/8, h = Kaiser-windowed sinc.
 * The parameters are those of the reference's chain as it runs here -- `audioresample` of GStreamer 1.14 at its
 * default quality, measured through its impulse response (tools/make_golden.py resampled; the fit leaves 5e-5
 * of the peak): cutoff 0.94 of the input's Nyquist frequency and 64 taps when the rate goes up, 0.921 of the
 * output's and 64 rate / 48000 taps (rounded up to a multiple of 8) when it goes down, Kaiser beta 8.4-8.5 (85 dB),
 * and a delay of one eighth of an INPUT sample; the last output sample is the last one whose position does not
 * pass the last input sample.  Rational ratios (44.1 kHz: 160 / 147) run from a polyphase table. */
static double
bessel_i0 (double x)
{
  double sum = 1., term = 1.;
  int k;
  for (k = 1; k < 60; k++) {
    term *= (x / (2. * k)) * (x / (2. * k));
    sum += term;
    if (term < 1e-18 * sum)
      break;
  }
  return sum;
}

typedef struct
{
  double fc, half, beta, i0b;
} rs_kernel;

static double
rs_tap (const rs_kernel * k, double d)
{                               /* h(d), d in input samples */
  const double u = d / k->half, arg = 2. * M_PI * k->fc * d;
  if (fabs (u) > 1.)
    return 0.;
  return 2. * k->fc * (fabs (arg) < 1e-12 ? 1. : sin (arg) / arg) * bessel_i0 (k->beta * sqrt (1. - u * u)) / k->i0b;
}

static unsigned long
gcd_ul (unsigned long a, unsigned long b)
{
  while (b) {
    const unsigned long t = a % b;
    a = b;
    b = t;
  }
  return a;
}

static int
resample_to_48k (wav_t * w)
{
  const double ratio = 48000. / w->rate;                        /* output samples per input sample */
  const double delay = 0.125;                                   /* input samples */
  rs_kernel k;
  const unsigned long g = gcd_ul (48000ul, (unsigned long) w->rate);
  const unsigned long L = 48000ul / g, M = (unsigned long) w->rate / g;   /* t_m = m M / L - delay */
  const size_t out_frames = w->frames ? (size_t) floor ((double) (w->frames - 1) * ratio) + 1 : 0;
  float *out = malloc ((out_frames ? out_frames : 1) * w->channels * sizeof (float));
  double *table = NULL;
  long K, j;
  size_t m;
  int c;
  if (!out)
    return -1;
  if (ratio >= 1.) {
    k.fc = 0.94 * 0.5;
    k.half = 32.15;
    k.beta = 8.49;
  } else {
    k.fc = 0.921 * 0.5 * ratio;
    k.half = 4. * ceil (64. / ratio / 8.);
    k.beta = 8.41;
  }
  k.i0b = bessel_i0 (k.beta);
  K = (long) ceil (k.half) + 1;                                 /* taps n = floor(t) - K + 1 .. floor(t) + K */
  if (L <= 4096) {                                              /* phase p = (m M) mod L: d = frac(t) + K - 1 - j */
    unsigned long p;
    table = malloc ((size_t) L * 2 * K * sizeof (double));
    if (!table) {
      free (out);
      return -1;
    }
    for (p = 0; p < L; p++) {
      /* t = q + p / L - delay with an integer q: floor and fraction of p / L - delay */
      const double tf = (double) p / (double) L - delay, fl = floor (tf), fr = tf - fl;
      for (j = 0; j < 2 * K; j++)
        table[p * 2 * K + j] = rs_tap (&k, fr + (double) (K - 1 - j));
    }
  }
  for (m = 0; m < out_frames; m++) {
    const unsigned long long mm = (unsigned long long) m * M;
    const unsigned long p = (unsigned long) (mm % L);
    const double tf = (double) p / (double) L - delay, fl = floor (tf);
    const long n_first = (long) (mm / L) + (long) fl - K + 1;    /* floor(t) - K + 1 */
    const double fr = tf - fl;
    double acc[2] = { 0., 0. };
    for (j = 0; j < 2 * K; j++) {
      const long n = n_first + j;
      double h;
      if (n < 0 || n >= (long) w->frames)
        continue;
      h = table ? table[p * 2 * K + j] : rs_tap (&k, fr + (double) (K - 1 - j));
      for (c = 0; c < w->channels; c++)
        acc[c] += h * w->samples[(size_t) n * w->channels + c];
    }
    for (c = 0; c < w->channels; c++)
      out[m * w->channels + c] = (float) acc[c];
  }
  free (table);
  free (w->samples);
  w->samples = out;
  w->frames = out_frames;
  w->rate = 48000;
  return 0;
}

static void
usage (const char *prog)
{
  printf ("Usage:\n  %s [OPTION...] REFFILE TESTFILE\n\n"
      "peaq computes the Objective Difference Grade based on ITU-R BS.1387-1 (but it\n"
      "does not meet its conformance requirements), on an AMD MI355X.\n\n"
      "  --version     print version information\n"
      "  --advanced    use advanced version\n"
      "  --basic       use basic version (default)\n"
      "  --level=DB    playback level in dB SPL of a full-scale sine (default 92)\n"
      "  --no-resample refuse files that are not sampled at 48 kHz instead of converting them\n"
      "  --device-resample convert files at other rates on the GPU instead of on the host\n"
      "                (the plain one-call mode only: not with --interval; both files at one rate)\n"
      "  --interval=S  also print ODG and DI read every S seconds through the files\n"
      "  --align[=SAMPLES] find the test file's delay within +-SAMPLES (48 kHz samples, 1..16384, default 4096)\n"
      "                on the GPU and compare the aligned parts (the plain one-call mode only)\n"
      "  --align-subsample[=SAMPLES] --align, and the sub-sample part of the delay too: estimated on a grid of 1/256\n"
      "                sample and removed from the test signal by a 65-tap shift filter; prints the fraction beside\n"
      "                the lag; --match-gain then measures after the shift (the plain one-call mode; not with --list)\n"
      "  --align-drift[=WINDOW] --align, and a steadily growing delay too (a second clock): the delay of every WINDOW\n"
      "                samples (4096..1048576, default 32768) is measured, one line fitted through them and the test\n"
      "                signal resampled along it; prints the line; excludes --align-subsample, which it subsumes\n"
      "                (the plain one-call mode; not with --list, --interval or --trace)\n"
      "  --align-track[=WINDOW] --align, and a delay that bends or steps too (two clocks one after the other, a loop\n"
      "                whose clock wanders, a player that re-synchronised): the delay of every WINDOW samples\n"
      "                (4096..1048576, default 16384) is measured and kept as a track, and the test signal is resampled\n"
      "                along it; prints the track's range; excludes --align-drift and --align-subsample, which it\n"
      "                subsumes (the plain one-call mode; not with --list, --interval or --trace)\n"
      "  --align-wide[=SECONDS[:waveform|envelope]] --align, with the delay searched within +-SECONDS (default 10, at most\n"
      "                21.8) coarse to fine: on copies decimated by up to 64, then within --align's range (default 4096)\n"
      "                around what that finds; envelope (default) also finds material without low frequencies; prints\n"
      "                the delay and a line with the coarse lag, the factor and the flags; excludes the other\n"
      "                --align-... options, --match-gain, --list, --interval and --trace\n"
      "  --align-steps[=WINDOW] --align-track, and steps of the delay inside a window too (a dropped or repeated block,\n"
      "                a concealed packet loss, an edit): every step of the track is located to the sample and the test\n"
      "                signal is cut along pieces that jump there; prints the track's range and each accepted step's\n"
      "                position and size; excludes --align-track, --align-drift and --align-subsample (the plain\n"
      "                one-call mode; not with --list, --interval or --trace)\n"
      "  --match-gain[=lsq|rms|polarity] match the test file's level (polarity) to the reference's on the GPU, after\n"
      "                --align if given, and print the gain applied (default lsq; the plain one-call mode and --list;\n"
      "                not with --interval or --trace)\n"
      "  --gain-per-channel  each channel its own gain\n"
      "  --max-gain=DB leave a pair unmatched whose gain is beyond +-DB (0 < DB <= 120, default 40)\n"
      "  --trace=FILE  also write the MOV layer's values of every frame (and, with --advanced, every filter-bank\n"
      "                block) to FILE as CSV (the plain one-call mode; with --advanced, --device-resample, --align)\n"
      "  --bands=FILE[:PLANES] also write the FFT path's values per frame, channel and critical band to FILE as CSV: a\n"
      "                noise-to-mask spectrogram.  PLANES: a comma-separated list of nmr, exc_ref, exc_test, detect,\n"
      "                steps (default nmr; with --advanced: nmr, exc_ref).  The header line carries the bands' centre\n"
      "                frequencies in Hz (the plain one-call mode; with --advanced, --device-resample, --align)\n"
      "  --fb-bands=FILE[:PLANES] with --advanced: also write the filter-bank path's values per block, channel and band\n"
      "                (40 bands) to FILE as CSV.  PLANES: a comma-separated list of moddiff, modwt, noiseloud, missing,\n"
      "                lindist, unsm_ref, unsm_test, exc_ref, exc_test, adapt_ref, adapt_test, mod_ref, mod_test\n"
      "                (default noiseloud).  The header line carries the bands' centre frequencies in Hz (the plain\n"
      "                one-call mode; with --device-resample, --align; a run of its own, like --bands)\n"
      "  --pattern-bands=FILE[:PLANES] basic version: also write the pattern layer's values per frame, channel and\n"
      "                critical band (109 bands) to FILE as CSV.  PLANES: a comma-separated list of moddiff1, moddiff2,\n"
      "                modwt, noiseloud, unsm_ref, unsm_test, exc_ref, exc_test, adapt_ref, adapt_test, mod_ref, mod_test,\n"
      "                avgloud_ref (default noiseloud).  The header line carries the bands' centre frequencies in Hz (the\n"
      "                plain one-call mode; with --device-resample, --align; a run of its own, like --bands; with\n"
      "                --advanced see --fb-bands)\n"
      "  --band-summary=FILE also write the pair's per-band summary to FILE as CSV: one line per channel and critical\n"
      "                band with the band's centre frequency in Hz, the band's sums over the counted frames (first to\n"
      "                last frame above the data boundary) and their denominators: nmr_sum, nmr_max, nmr_disturbed,\n"
      "                exc_ref_sum and, in the basic version, exc_test_sum, moddiff1_wsum, moddiff2_wsum, noiseloud_sum\n"
      "                (the plain one-call mode; with --advanced, --device-resample, --align; a run of its own, like\n"
      "                --bands)\n"
      "  --fb-band-summary=FILE with --advanced: also write the filter-bank path's per-band summary (40 bands, the ones\n"
      "                behind RmsModDiff, RmsNoiseLoudAsym and AvgLinDist) to FILE as CSV: one line per channel and band\n"
      "                with the band's centre frequency in Hz, the band's sums over the counted blocks (first to last\n"
      "                block above the data boundary) and their denominators: exc_ref_sum, exc_test_sum, moddiff_wsum,\n"
      "                moddiff_sq, noiseloud_sq, missing_sq, lindist_sum (the plain one-call mode; with\n"
      "                --device-resample, --align; a run of its own, like --bands)\n"
      "  --windows=S[:HOP] basic version: also print, before the two result lines, the score of every window of S\n"
      "                seconds taken every HOP seconds (default S) through the files as scored, the last one ending with\n"
      "                them: one line `window START_S END_S FRAMES ODG DI` each.  A window reads the frames it covers\n"
      "                in the context of the running stream, not the excerpt from a cold start (the plain one-call mode;\n"
      "                with --device-resample, --align; a run of its own, like --bands)\n"
      "  --spans=S[:HOP] with --advanced: the same for the advanced version, one line `span START_S END_S FRAMES BLOCKS\n"
      "                ODG DI` each: a span reads the FFT frames and the filter-bank blocks it covers in the context of\n"
      "                the running stream (the plain one-call mode; with --device-resample, --align; a run of its own)\n"
      "  --list=FILE   score the pairs listed in FILE, one REF<TAB>TEST per line, instead of REFFILE TESTFILE;\n"
      "                prints REF<TAB>TEST<TAB>ODG<TAB>DI per pair (with --advanced, --level, --align)\n"
      "  --no-share-refs with --list: read and upload a reference file again for every line that names it\n", prog);
}

/* --trace=FILE: the pair through peaq_run_pair_trace, its records as CSV -- a header line, then one line per FFT frame
 * (kind "frame") and, in the advanced version, per filter-bank block (kind "block"); every value as %.17g, which reads
 * back to the same double.  Columns a kind does not have stay empty.  Prints the delay line of --align. */
static int
write_trace (const char *path, peaq_ctx *ctx, int advanced, double level, uint32_t rate, uint32_t align_lag,
    const wav_t *ref, const wav_t *test, peaq_result *r)
{
  /* enough for any cut: the counts of the two signals at 48 kHz */
  const uint64_t n48[2] = { rate == 48000 ? ref->frames : peaq_resampled_length (ref->frames, rate),
    rate == 48000 ? test->frames : peaq_resampled_length (test->frames, rate) };
  const size_t frame_cap = (size_t) peaq_frame_count (n48[0], n48[1], 0) + 1;
  const size_t block_cap = advanced ? (size_t) peaq_frame_count (n48[0], n48[1], 1) + 1 : 0;
  peaq_frame_trace *fr = malloc (frame_cap * sizeof *fr);
  peaq_block_trace *bl = advanced ? malloc (block_cap * sizeof *bl) : NULL;
  uint32_t nf = 0, nb = 0, k;
  peaq_delay delay;
  size_t fb = 0, bb = 0;
  int c, v, rc = 1;
  FILE *f;
  if (!fr || (advanced && !bl)) {
    printf ("Error: out of memory for the trace\n");
    goto done;
  }
  peaq_trace_sizes (&fb, &bb);
  if (fb != sizeof *fr || bb != sizeof *bl) {
    printf ("Error: the library's trace records are not this program's\n");
    goto done;
  }
  if (peaq_run_pair_trace (ctx, advanced, ref->channels, level, rate, align_lag, ref->samples, ref->frames, test->samples,
          test->frames, fr, frame_cap, &nf, bl, block_cap, &nb, &delay, r) != PEAQ_OK) {
    printf ("Error: %s\n", peaq_last_error ());
    goto done;
  }
  if (align_lag)
    printf ("Delay: %d samples (correlation %.3f)\n", (int) delay.lag, delay.norm > 0. ? delay.peak / delay.norm : 0.);
  if (!(f = fopen (path, "w"))) {
    printf ("Error: cannot write %s\n", path);
    goto done;
  }
  fprintf (f, "kind,index,flags");
  for (c = 0; c < 2; c++)
    for (v = 0; v < 6; v++)
      fprintf (f, ",ch%d_v%d", c, v);
  fprintf (f, ",p_detect,steps\n");
  for (k = 0; k < nf; k++) {
    fprintf (f, "frame,%u,%u", fr[k].frame, fr[k].flags);
    for (c = 0; c < 2; c++)
      for (v = 0; v < 6; v++)
        fprintf (f, ",%.17g", fr[k].ch[c][v]);
    fprintf (f, ",%.17g,%.17g\n", fr[k].p_detect, fr[k].steps);
  }
  for (k = 0; k < nb; k++) {
    fprintf (f, "block,%u,%u", bl[k].block, bl[k].flags);
    for (c = 0; c < 2; c++) {
      for (v = 0; v < 5; v++)
        fprintf (f, ",%.17g", bl[k].ch[c][v]);
      fprintf (f, ",");
    }
    fprintf (f, ",,\n");
  }
  if (fclose (f)) {
    printf ("Error: cannot write %s\n", path);
    goto done;
  }
  rc = 0;
done:
  free (fr);
  free (bl);
  return rc;
}

/* The three band-row outputs, --bands, --fb-bands and --pattern-bands =FILE[:PLANES]: the planes of each by name, in the
 * order of their bits (PEAQ_BAND_*, PEAQ_FB_BAND_*, PEAQ_PAT_BAND_*), and what a row of each is counted in. */
enum band_kind { BANDS_FFT, BANDS_FB, BANDS_PATTERN };
static const char *const band_plane_names[] = { "nmr", "exc_ref", "exc_test", "detect", "steps" };
static const char *const fb_band_plane_names[] = { "moddiff", "modwt", "noiseloud", "missing", "lindist",
  "unsm_ref", "unsm_test", "exc_ref", "exc_test", "adapt_ref", "adapt_test", "mod_ref", "mod_test" };
static const char *const pattern_band_plane_names[] = { "moddiff1", "moddiff2", "modwt", "noiseloud",
  "unsm_ref", "unsm_test", "exc_ref", "exc_test", "adapt_ref", "adapt_test", "mod_ref", "mod_test", "avgloud_ref" };
static const struct {
  const char *unit;             /* the header's first word */
  const char *const *names;
  int n_names;
} band_kinds[] = {
  { "frame", band_plane_names, 5 },
  { "block", fb_band_plane_names, 13 },
  { "frame", pattern_band_plane_names, 13 },
};

/* a comma-separated list of plane names -> mask; 0 if a name is not one */
static uint32_t
parse_planes (const char *list, const char *const *names, int n_names)
{
  uint32_t mask = 0;
  while (*list) {
    const size_t n = strcspn (list, ",");
    int k, hit = -1;
    for (k = 0; k < n_names; k++)
      if (strlen (names[k]) == n && !strncmp (list, names[k], n))
        hit = k;
    if (hit < 0)
      return 0;
    mask |= 1u << hit;
    list += n;
    if (*list == ',' && !*++list)
      return 0;
  }
  return mask;
}

/* The pair through peaq_run_pair_bands, _fb_bands or _pattern_bands, its rows as CSV -- a header line (frame or block,
 * channel, plane, then the bands' centre frequencies in Hz), then one line per (frame or block, channel, plane) with
 * the band values; every value as %.17g, which reads back to the same double.  Prints the delay line of --align.
 * `advanced`: BANDS_FFT only (the filter bank belongs to the advanced version, the pattern layer to the basic one). */
static int
write_band_rows (enum band_kind kind, const char *path, uint32_t planes, peaq_ctx *ctx, int advanced, double level,
    uint32_t rate, uint32_t align_lag, const wav_t *ref, const wav_t *test, peaq_result *r)
{
  const uint64_t n48[2] = { rate == 48000 ? ref->frames : peaq_resampled_length (ref->frames, rate),
    rate == 48000 ? test->frames : peaq_resampled_length (test->frames, rate) };
  const size_t cap = (size_t) peaq_frame_count (n48[0], n48[1], kind == BANDS_FB) + 1;
  const int adv = kind == BANDS_FFT && advanced, ch = ref->channels;
  const int count = kind == BANDS_FB ? peaq_fb_band_count () : peaq_band_count (adv);
  const int row = kind == BANDS_FB ? count : peaq_band_row (adv);
  const char *const *names = band_kinds[kind].names;
  const int n_names = band_kinds[kind].n_names;
  int n_planes = 0, c, k, b, slot, rc = 1, ok = 0;
  double *rows, *fc;
  uint32_t n = 0, i;
  peaq_delay delay;
  FILE *out;
  for (k = 0; k < n_names; k++)
    n_planes += (planes >> k) & 1;
  rows = malloc (cap * ch * (n_planes ? n_planes : 1) * row * sizeof *rows);
  fc = malloc (count * sizeof *fc);
  if (!rows || !fc) {
    printf ("Error: out of memory for the band trace\n");
    goto done;
  }
  switch (kind) {
  case BANDS_FFT:
    ok = peaq_band_tables (adv, fc, NULL) == PEAQ_OK &&
        peaq_run_pair_bands (ctx, adv, ch, level, rate, align_lag, ref->samples, ref->frames, test->samples, test->frames,
            planes, rows, cap, &n, &delay, r) == PEAQ_OK;
    break;
  case BANDS_FB:
    ok = peaq_fb_band_tables (fc, NULL) == PEAQ_OK &&
        peaq_run_pair_fb_bands (ctx, ch, level, rate, align_lag, ref->samples, ref->frames, test->samples, test->frames,
            planes, rows, cap, &n, &delay, r) == PEAQ_OK;
    break;
  case BANDS_PATTERN:
    ok = peaq_pattern_band_tables (fc, NULL) == PEAQ_OK &&
        peaq_run_pair_pattern_bands (ctx, ch, level, rate, align_lag, ref->samples, ref->frames, test->samples,
            test->frames, planes, rows, cap, &n, &delay, r) == PEAQ_OK;
    break;
  }
  if (!ok) {
    printf ("Error: %s\n", peaq_last_error ());
    goto done;
  }
  if (align_lag)
    printf ("Delay: %d samples (correlation %.3f)\n", (int) delay.lag, delay.norm > 0. ? delay.peak / delay.norm : 0.);
  if (!(out = fopen (path, "w"))) {
    printf ("Error: cannot write %s\n", path);
    goto done;
  }
  fprintf (out, "%s,channel,plane", band_kinds[kind].unit);
  for (b = 0; b < count; b++)
    fprintf (out, ",%.17g", fc[b]);
  fprintf (out, "\n");
  for (i = 0; i < n; i++)
    for (c = 0; c < ch; c++)
      for (k = 0, slot = 0; k < n_names; k++) {
        const double *v;
        if (!((planes >> k) & 1))
          continue;
        v = rows + (((size_t) i * ch + c) * n_planes + slot++) * row;
        fprintf (out, "%u,%d,%s", i, c, names[k]);
        for (b = 0; b < count; b++)
          fprintf (out, ",%.17g", v[b]);
        fprintf (out, "\n");
      }
  if (fclose (out)) {
    printf ("Error: cannot write %s\n", path);
    goto done;
  }
  rc = 0;
done:
  free (rows);
  free (fc);
  return rc;
}

/* the rows of --band-summary=FILE by name, in row order (PEAQ_BAND_SUMMARY_*), and the name of each row's denominator */
enum { n_band_summary_rows = 8 };
static const char *const band_summary_row_names[n_band_summary_rows] = { "nmr_sum", "nmr_max", "nmr_disturbed",
  "exc_ref_sum", "exc_test_sum", "moddiff1_wsum", "moddiff2_wsum", "noiseloud_sum" };

/* --band-summary=FILE: the pair through peaq_run_pair_band_summary, its rows as CSV -- a header line, then one line per
 * (channel, band): the band's centre frequency in Hz, the band's value of every row, then the denominators the rows
 * share (counted: the number of counted frames; in the basic version also modwt_sum, the sum of the frames' weights
 * under the two modulation-difference rows, and loud_frames, the number of frames under noiseloud_sum); every value as
 * %.17g, which reads back to the same double.  Prints the delay line of --align. */
static int
write_band_summary (const char *path, peaq_ctx *ctx, int advanced, double level, uint32_t rate, uint32_t align_lag,
    const wav_t *ref, const wav_t *test, peaq_result *r)
{
  const int count = peaq_band_count (advanced), row = peaq_band_row (advanced), n_rows = peaq_band_summary_rows (advanced);
  const int ch = ref->channels;
  int c, k, b, rc = 1;
  double *rows, *fc;
  peaq_delay delay;
  FILE *out;
  rows = malloc ((size_t) ch * n_rows * row * sizeof *rows);
  fc = malloc (count * sizeof *fc);
  if (!rows || !fc) {
    printf ("Error: out of memory for the band summary\n");
    goto done;
  }
  if (peaq_band_tables (advanced, fc, NULL) != PEAQ_OK ||
      peaq_run_pair_band_summary (ctx, advanced, ch, level, rate, align_lag, ref->samples, ref->frames, test->samples,
          test->frames, rows, &delay, r) != PEAQ_OK) {
    printf ("Error: %s\n", peaq_last_error ());
    goto done;
  }
  if (align_lag)
    printf ("Delay: %d samples (correlation %.3f)\n", (int) delay.lag, delay.norm > 0. ? delay.peak / delay.norm : 0.);
  if (!(out = fopen (path, "w"))) {
    printf ("Error: cannot write %s\n", path);
    goto done;
  }
  fprintf (out, "channel,band,fc");
  for (k = 0; k < n_rows; k++)
    fprintf (out, ",%s", band_summary_row_names[k]);
  fprintf (out, advanced ? ",counted\n" : ",counted,modwt_sum,loud_frames\n");
  for (c = 0; c < ch; c++) {
    const double *v = rows + (size_t) c * n_rows * row;
    for (b = 0; b < count; b++) {
      fprintf (out, "%d,%d,%.17g", c, b, fc[b]);
      for (k = 0; k < n_rows; k++)
        fprintf (out, ",%.17g", v[k * row + b]);
      fprintf (out, ",%.17g", v[PEAQ_BAND_SUMMARY_NMR_SUM * row + count]);
      if (!advanced)
        fprintf (out, ",%.17g,%.17g", v[PEAQ_BAND_SUMMARY_MODDIFF1_WSUM * row + count],
            v[PEAQ_BAND_SUMMARY_NOISELOUD_SUM * row + count]);
      fprintf (out, "\n");
    }
  }
  if (fclose (out)) {
    printf ("Error: cannot write %s\n", path);
    goto done;
  }
  rc = 0;
done:
  free (rows);
  free (fc);
  return rc;
}

/* the rows of --fb-band-summary=FILE by name, in row order (PEAQ_FB_BAND_SUMMARY_*) */
enum { n_fb_band_summary_rows = 7 };
static const char *const fb_band_summary_row_names[n_fb_band_summary_rows] = { "exc_ref_sum", "exc_test_sum",
  "moddiff_wsum", "moddiff_sq", "noiseloud_sq", "missing_sq", "lindist_sum" };

/* --fb-band-summary=FILE: the pair through peaq_run_pair_fb_band_summary, its rows as CSV -- a header line, then one
 * line per (channel, band): the band's centre frequency in Hz, the band's value of the seven rows, then the rows'
 * denominators (counted: the number of counted blocks; modwt_sum and modwt_sq_sum, the sums of W and W^2 under the two
 * modulation-difference rows; loud_blocks, the number of blocks under the last three rows); every value as %.17g, which
 * reads back to the same double.  Prints the delay line of --align. */
static int
write_fb_band_summary (const char *path, peaq_ctx *ctx, double level, uint32_t rate, uint32_t align_lag,
    const wav_t *ref, const wav_t *test, peaq_result *r)
{
  const int count = peaq_fb_band_count (), row = peaq_fb_band_summary_row (), n_rows = peaq_fb_band_summary_rows ();
  const int ch = ref->channels;
  int c, k, b, rc = 1;
  double *rows, *fc;
  peaq_delay delay;
  FILE *out;
  rows = malloc ((size_t) ch * n_rows * row * sizeof *rows);
  fc = malloc (count * sizeof *fc);
  if (!rows || !fc) {
    printf ("Error: out of memory for the band summary\n");
    goto done;
  }
  if (peaq_fb_band_tables (fc, NULL) != PEAQ_OK ||
      peaq_run_pair_fb_band_summary (ctx, ch, level, rate, align_lag, ref->samples, ref->frames, test->samples,
          test->frames, rows, &delay, r) != PEAQ_OK) {
    printf ("Error: %s\n", peaq_last_error ());
    goto done;
  }
  if (align_lag)
    printf ("Delay: %d samples (correlation %.3f)\n", (int) delay.lag, delay.norm > 0. ? delay.peak / delay.norm : 0.);
  if (!(out = fopen (path, "w"))) {
    printf ("Error: cannot write %s\n", path);
    goto done;
  }
  fprintf (out, "channel,band,fc");
  for (k = 0; k < n_rows; k++)
    fprintf (out, ",%s", fb_band_summary_row_names[k]);
  fprintf (out, ",counted,modwt_sum,modwt_sq_sum,loud_blocks\n");
  for (c = 0; c < ch; c++) {
    const double *v = rows + (size_t) c * n_rows * row;
    for (b = 0; b < count; b++) {
      fprintf (out, "%d,%d,%.17g", c, b, fc[b]);
      for (k = 0; k < n_rows; k++)
        fprintf (out, ",%.17g", v[k * row + b]);
      fprintf (out, ",%.17g,%.17g,%.17g,%.17g\n", v[PEAQ_FB_BAND_SUMMARY_EXC_REF_SUM * row + count],
          v[PEAQ_FB_BAND_SUMMARY_MODDIFF_WSUM * row + count], v[PEAQ_FB_BAND_SUMMARY_MODDIFF_SQ * row + count],
          v[PEAQ_FB_BAND_SUMMARY_NOISELOUD_SQ * row + count]);
    }
  }
  if (fclose (out)) {
    printf ("Error: cannot write %s\n", path);
    goto done;
  }
  rc = 0;
done:
  free (rows);
  free (fc);
  return rc;
}

/* --windows=S[:HOP]: the pair through peaq_run_pair_windows with the sliding windows of the scored length -- starts
 * every `hop` samples from 0, `length` samples each, up to the first that reaches the end, which ends there -- one line
 * per window.  With --align the scored length is the common part, known after the run: the windows are laid over the
 * longer file and those of the common part printed (a window that reaches the end of the scored signals reads through
 * their last frame wherever its own end lies).  Prints the delay line of --align.
 * spans != 0: --spans=S[:HOP], the same through peaq_run_pair_adv_spans, the lines with the count of blocks as well. */
static int
print_windows (int spans, uint32_t length, uint32_t hop, peaq_ctx *ctx, double level, uint32_t rate, uint32_t align_lag,
    const wav_t *ref, const wav_t *test, peaq_result *r)
{
  const uint32_t n_ref = rate == 48000 ? (uint32_t) ref->frames : peaq_resampled_length (ref->frames, rate);
  const uint32_t n_test = rate == 48000 ? (uint32_t) test->frames : peaq_resampled_length (test->frames, rate);
  uint32_t n = n_ref > n_test ? n_ref : n_test;
  size_t n_windows = 1, k;
  peaq_window *w;
  peaq_result *rows;
  peaq_delay delay;
  int rc = 1;
  if (n > length)
    n_windows += ((size_t) n - length + hop - 1) / hop;
  if (n_windows > PEAQ_WINDOWS_MAX) {
    printf ("Error: %zu %s are more than %d\n", n_windows, spans ? "spans" : "windows", PEAQ_WINDOWS_MAX);
    return 1;
  }
  w = malloc (n_windows * sizeof *w);
  rows = malloc (n_windows * sizeof *rows);
  if (!w || !rows) {
    printf ("Error: out of memory for the windows\n");
    goto done;
  }
  for (k = 0; k < n_windows; k++) {
    w[k].start = (uint32_t) (k * hop);
    w[k].length = length;
  }
  if ((spans ? peaq_run_pair_adv_spans : peaq_run_pair_windows) (ctx, ref->channels, level, rate, align_lag, ref->samples,
          ref->frames, test->samples, test->frames, w, (int) n_windows, rows, &delay, r) != PEAQ_OK) {
    printf ("Error: %s\n", peaq_last_error ());
    goto done;
  }
  if (align_lag) {
    uint32_t skip_ref, skip_test;
    printf ("Delay: %d samples (correlation %.3f)\n", (int) delay.lag, delay.norm > 0. ? delay.peak / delay.norm : 0.);
    peaq_aligned_lengths (delay.lag, n_ref, n_test, &skip_ref, &skip_test, &n);
  }
  for (k = 0; k < n_windows; k++) {
    const uint64_t end = (uint64_t) w[k].start + length;
    if (spans)
      printf ("span %.3f %.3f %.0f %.0f %.3f %.3f\n", w[k].start / 48000., (end < n ? end : n) / 48000., rows[k].frames,
          rows[k].fb_blocks, rows[k].odg, rows[k].di);
    else
      printf ("window %.3f %.3f %.0f %.3f %.3f\n", w[k].start / 48000., (end < n ? end : n) / 48000., rows[k].frames,
          rows[k].odg, rows[k].di);
    if (end >= n)
      break;
  }
  rc = 0;
done:
  free (w);
  free (rows);
  return rc;
}

int
main (int argc, char **argv)
{
  int advanced = 0, i, nfiles = 0, rc, allow_resample = 1, device_resample = 0;
  uint32_t device_rate = 0;     /* != 0: both files stay at this rate, peaq_run_pair_rate converts them */
  uint32_t align_lag = 0;       /* != 0: --align, peaq_run_pair_aligned */
  int subsample = 0;            /* --align-subsample: peaq_run_pair_subsample (implies --align) */
  peaq_subdelay subdelay;
  uint32_t drift_window = 0;    /* != 0: --align-drift, peaq_run_pair_drift (implies --align) */
  peaq_drift drift;
  uint32_t track_window = 0;    /* != 0: --align-track, peaq_run_pair_track (implies --align) */
  peaq_track track;
  uint32_t steps_window = 0;    /* != 0: --align-steps, peaq_run_pair_steps (implies --align) */
  uint32_t wide_offset = 0;     /* != 0: --align-wide, peaq_run_pair_wide (implies --align) */
  int wide_mode = PEAQ_WIDE_ENVELOPE;
  peaq_delay delay;
  peaq_gain gain;
  int gain_mode = 0, gain_per_channel = 0;   /* != 0: --match-gain, peaq_run_pair_matched */
  double max_gain_db = 40.;
  double level = 92., interval_s = 0.;
  const char *files[2] = { NULL, NULL };
  const char *list_path = NULL, *trace_path = NULL;
  char *bands_path = NULL;      /* --bands=FILE[:PLANES], peaq_run_pair_bands */
  uint32_t band_planes = PEAQ_BAND_NMR;
  char *fb_bands_path = NULL;   /* --fb-bands=FILE[:PLANES], peaq_run_pair_fb_bands */
  uint32_t fb_band_planes = PEAQ_FB_BAND_NOISELOUD;
  char *pattern_bands_path = NULL;   /* --pattern-bands=FILE[:PLANES], peaq_run_pair_pattern_bands */
  uint32_t pattern_band_planes = PEAQ_PAT_BAND_NOISELOUD;
  const char *band_summary_path = NULL;   /* --band-summary=FILE, peaq_run_pair_band_summary */
  const char *fb_band_summary_path = NULL;   /* --fb-band-summary=FILE, peaq_run_pair_fb_band_summary */
  uint32_t windows_length = 0, windows_hop = 0;   /* != 0: --windows=S[:HOP], peaq_run_pair_windows */
  uint32_t spans_length = 0, spans_hop = 0;       /* != 0: --spans=S[:HOP], peaq_run_pair_adv_spans (with --advanced) */
  int share_refs = 1;
  wav_t ref, test;
  peaq_ctx *ctx = NULL;
  peaq_session *s = NULL;
  peaq_result r;
  size_t pos;

  for (i = 1; i < argc; i++) {
    if (!strcmp (argv[i], "--advanced"))
      advanced = 1;
    else if (!strcmp (argv[i], "--basic"))
      advanced = 0;
    else if (!strncmp (argv[i], "--level=", 8))
      level = atof (argv[i] + 8);
    else if (!strcmp (argv[i], "--no-resample"))
      allow_resample = 0;
    else if (!strcmp (argv[i], "--device-resample"))
      device_resample = 1;
    else if (!strcmp (argv[i], "--align"))
      align_lag = 4096;
    else if (!strncmp (argv[i], "--align=", 8)) {
      char *end;
      const long v = strtol (argv[i] + 8, &end, 10);
      if (*end || end == argv[i] + 8 || v < 1 || v > 16384) {
        fprintf (stderr, "Failed to initialize: invalid alignment range %s (1 .. 16384 samples)\n", argv[i] + 8);
        return 1;
      }
      align_lag = (uint32_t) v;
    }
    else if (!strcmp (argv[i], "--align-subsample")) {
      subsample = 1;
      if (!align_lag)
        align_lag = 4096;
    } else if (!strncmp (argv[i], "--align-subsample=", 18)) {
      char *end;
      const long v = strtol (argv[i] + 18, &end, 10);
      if (*end || end == argv[i] + 18 || v < 1 || v > 16384) {
        fprintf (stderr, "Failed to initialize: invalid alignment range %s (1 .. 16384 samples)\n", argv[i] + 18);
        return 1;
      }
      subsample = 1;
      align_lag = (uint32_t) v;
    }
    else if (!strcmp (argv[i], "--align-drift")) {
      drift_window = 32768;
      if (!align_lag)
        align_lag = 4096;
    } else if (!strncmp (argv[i], "--align-drift=", 14)) {
      char *end;
      const long v = strtol (argv[i] + 14, &end, 10);
      if (*end || end == argv[i] + 14 || v < 4096 || v > 1048576) {
        fprintf (stderr, "Failed to initialize: invalid drift window %s (4096 .. 1048576 samples)\n", argv[i] + 14);
        return 1;
      }
      drift_window = (uint32_t) v;
      if (!align_lag)
        align_lag = 4096;
    }
    else if (!strcmp (argv[i], "--align-track")) {
      track_window = 16384;
      if (!align_lag)
        align_lag = 4096;
    } else if (!strncmp (argv[i], "--align-track=", 14)) {
      char *end;
      const long v = strtol (argv[i] + 14, &end, 10);
      if (*end || end == argv[i] + 14 || v < 4096 || v > 1048576) {
        fprintf (stderr, "Failed to initialize: invalid track window %s (4096 .. 1048576 samples)\n", argv[i] + 14);
        return 1;
      }
      track_window = (uint32_t) v;
      if (!align_lag)
        align_lag = 4096;
    }
    else if (!strcmp (argv[i], "--align-steps")) {
      steps_window = 16384;
      if (!align_lag)
        align_lag = 4096;
    } else if (!strncmp (argv[i], "--align-steps=", 14)) {
      char *end;
      const long v = strtol (argv[i] + 14, &end, 10);
      if (*end || end == argv[i] + 14 || v < 4096 || v > 1048576) {
        fprintf (stderr, "Failed to initialize: invalid steps window %s (4096 .. 1048576 samples)\n", argv[i] + 14);
        return 1;
      }
      steps_window = (uint32_t) v;
      if (!align_lag)
        align_lag = 4096;
    }
    else if (!strcmp (argv[i], "--align-wide")) {
      wide_offset = 480000;
      if (!align_lag)
        align_lag = 4096;
    } else if (!strncmp (argv[i], "--align-wide=", 13)) {
      char *end;
      const double v = strtod (argv[i] + 13, &end);
      if (end == argv[i] + 13 || !(v > 0. && v <= 21.8) || (uint32_t) (v * 48000. + 0.5) < 1 ||
          (*end && strcmp (end, ":envelope") && strcmp (end, ":waveform"))) {
        fprintf (stderr, "Failed to initialize: invalid wide offset %s (SECONDS[:waveform|envelope], up to 21.8 s)\n", argv[i] + 13);
        return 1;
      }
      wide_offset = (uint32_t) (v * 48000. + 0.5);
      wide_mode = !strcmp (end, ":waveform") ? PEAQ_WIDE_WAVEFORM : PEAQ_WIDE_ENVELOPE;
      if (!align_lag)
        align_lag = 4096;
    }
    else if (!strcmp (argv[i], "--match-gain") || !strcmp (argv[i], "--match-gain=lsq"))
      gain_mode = PEAQ_GAIN_LSQ;
    else if (!strcmp (argv[i], "--match-gain=rms"))
      gain_mode = PEAQ_GAIN_RMS;
    else if (!strcmp (argv[i], "--match-gain=polarity"))
      gain_mode = PEAQ_GAIN_POLARITY;
    else if (!strncmp (argv[i], "--match-gain=", 13)) {
      fprintf (stderr, "Failed to initialize: invalid gain mode %s (lsq, rms or polarity)\n", argv[i] + 13);
      return 1;
    }
    else if (!strcmp (argv[i], "--gain-per-channel"))
      gain_per_channel = 1;
    else if (!strncmp (argv[i], "--max-gain=", 11)) {
      char *end;
      max_gain_db = strtod (argv[i] + 11, &end);
      if (*end || end == argv[i] + 11 || !(max_gain_db > 0. && max_gain_db <= 120.)) {
        fprintf (stderr, "Failed to initialize: invalid gain limit %s (0 < DB <= 120)\n", argv[i] + 11);
        return 1;
      }
    }
    else if (!strncmp (argv[i], "--interval=", 11)) {
      char *end;
      interval_s = strtod (argv[i] + 11, &end);
      if (*end || !(interval_s * 48000. >= 0.5 && interval_s * 48000. < 4294967295.)) {
        fprintf (stderr, "Failed to initialize: invalid interval %s\n", argv[i] + 11);
        return 1;
      }
    }
    else if (!strncmp (argv[i], "--list=", 7))
      list_path = argv[i] + 7;
    else if (!strcmp (argv[i], "--no-share-refs"))
      share_refs = 0;
    else if (!strcmp (argv[i], "--trace") || !strcmp (argv[i], "--trace=")) {
      fprintf (stderr, "Failed to initialize: --trace needs a file name (--trace=FILE)\n");
      return 1;
    } else if (!strncmp (argv[i], "--trace=", 8))
      trace_path = argv[i] + 8;
    else if (!strcmp (argv[i], "--bands") || !strcmp (argv[i], "--bands=") || !strncmp (argv[i], "--bands=:", 9)) {
      fprintf (stderr, "Failed to initialize: --bands needs a file name (--bands=FILE[:PLANES])\n");
      return 1;
    } else if (!strncmp (argv[i], "--bands=", 8)) {
      /* what follows the last colon is the plane list if every name in it is one; a file name otherwise */
      char *colon = strrchr (argv[i] + 8, ':');
      bands_path = argv[i] + 8;
      if (colon && !colon[1]) {
        fprintf (stderr, "Failed to initialize: --bands: no plane after the colon (nmr, exc_ref, exc_test, detect, steps)\n");
        return 1;
      }
      if (colon && parse_planes (colon + 1, band_kinds[BANDS_FFT].names, band_kinds[BANDS_FFT].n_names)) {
        band_planes = parse_planes (colon + 1, band_kinds[BANDS_FFT].names, band_kinds[BANDS_FFT].n_names);
        *colon = 0;
      }
    }
    else if (!strcmp (argv[i], "--fb-bands") || !strcmp (argv[i], "--fb-bands=") || !strncmp (argv[i], "--fb-bands=:", 12)) {
      fprintf (stderr, "Failed to initialize: --fb-bands needs a file name (--fb-bands=FILE[:PLANES])\n");
      return 1;
    } else if (!strncmp (argv[i], "--fb-bands=", 11)) {
      /* what follows the last colon is the plane list if every name in it is one; a file name otherwise */
      char *colon = strrchr (argv[i] + 11, ':');
      fb_bands_path = argv[i] + 11;
      if (colon && !colon[1]) {
        fprintf (stderr, "Failed to initialize: --fb-bands: no plane after the colon (moddiff, modwt, noiseloud, missing, lindist, unsm_ref, unsm_test, exc_ref, exc_test, adapt_ref, adapt_test, mod_ref, mod_test)\n");
        return 1;
      }
      if (colon && parse_planes (colon + 1, band_kinds[BANDS_FB].names, band_kinds[BANDS_FB].n_names)) {
        fb_band_planes = parse_planes (colon + 1, band_kinds[BANDS_FB].names, band_kinds[BANDS_FB].n_names);
        *colon = 0;
      }
    }
    else if (!strcmp (argv[i], "--pattern-bands") || !strcmp (argv[i], "--pattern-bands=") || !strncmp (argv[i], "--pattern-bands=:", 17)) {
      fprintf (stderr, "Failed to initialize: --pattern-bands needs a file name (--pattern-bands=FILE[:PLANES])\n");
      return 1;
    } else if (!strncmp (argv[i], "--pattern-bands=", 16)) {
      /* what follows the last colon is the plane list if every name in it is one; a file name otherwise */
      char *colon = strrchr (argv[i] + 16, ':');
      pattern_bands_path = argv[i] + 16;
      if (colon && !colon[1]) {
        fprintf (stderr, "Failed to initialize: --pattern-bands: no plane after the colon (moddiff1, moddiff2, modwt, noiseloud, unsm_ref, unsm_test, exc_ref, exc_test, adapt_ref, adapt_test, mod_ref, mod_test, avgloud_ref)\n");
        return 1;
      }
      if (colon && parse_planes (colon + 1, band_kinds[BANDS_PATTERN].names, band_kinds[BANDS_PATTERN].n_names)) {
        pattern_band_planes = parse_planes (colon + 1, band_kinds[BANDS_PATTERN].names, band_kinds[BANDS_PATTERN].n_names);
        *colon = 0;
      }
    }
    else if (!strcmp (argv[i], "--band-summary") || !strcmp (argv[i], "--band-summary=")) {
      fprintf (stderr, "Failed to initialize: --band-summary needs a file name (--band-summary=FILE)\n");
      return 1;
    } else if (!strncmp (argv[i], "--band-summary=", 15))
      band_summary_path = argv[i] + 15;
    else if (!strcmp (argv[i], "--fb-band-summary") || !strcmp (argv[i], "--fb-band-summary=")) {
      fprintf (stderr, "Failed to initialize: --fb-band-summary needs a file name (--fb-band-summary=FILE)\n");
      return 1;
    } else if (!strncmp (argv[i], "--fb-band-summary=", 18))
      fb_band_summary_path = argv[i] + 18;
    else if (!strcmp (argv[i], "--windows") || !strcmp (argv[i], "--windows=")) {
      fprintf (stderr, "Failed to initialize: --windows needs a length in seconds (--windows=SECONDS[:HOP_SECONDS])\n");
      return 1;
    } else if (!strncmp (argv[i], "--windows=", 10)) {
      char *end;
      const double len_s = strtod (argv[i] + 10, &end);
      double hop_s = len_s;
      if (end != argv[i] + 10 && *end == ':' && end[1])
        hop_s = strtod (end + 1, &end);
      if (end == argv[i] + 10 || *end || !(len_s * 48000. >= 0.5 && len_s * 48000. < 4294967295.) ||
          !(hop_s * 48000. >= 0.5 && hop_s * 48000. < 4294967295.)) {
        fprintf (stderr, "Failed to initialize: invalid windows %s\n", argv[i] + 10);
        return 1;
      }
      windows_length = (uint32_t) llround (len_s * 48000.);
      windows_hop = (uint32_t) llround (hop_s * 48000.);
    }
    else if (!strcmp (argv[i], "--spans") || !strcmp (argv[i], "--spans=")) {
      fprintf (stderr, "Failed to initialize: --spans needs a length in seconds (--spans=SECONDS[:HOP_SECONDS])\n");
      return 1;
    } else if (!strncmp (argv[i], "--spans=", 8)) {
      char *end;
      const double len_s = strtod (argv[i] + 8, &end);
      double hop_s = len_s;
      if (end != argv[i] + 8 && *end == ':' && end[1])
        hop_s = strtod (end + 1, &end);
      if (end == argv[i] + 8 || *end || !(len_s * 48000. >= 0.5 && len_s * 48000. < 4294967295.) ||
          !(hop_s * 48000. >= 0.5 && hop_s * 48000. < 4294967295.)) {
        fprintf (stderr, "Failed to initialize: invalid spans %s\n", argv[i] + 8);
        return 1;
      }
      spans_length = (uint32_t) llround (len_s * 48000.);
      spans_hop = (uint32_t) llround (hop_s * 48000.);
    }
    else if (!strcmp (argv[i], "--version")) {
      printf ("peaq (gstpeaq_amd) %s\n", peaq_version ());
      return 0;
    } else if (!strcmp (argv[i], "--help") || !strcmp (argv[i], "-h")) {
      usage (argv[0]);
      return 0;
    } else if (argv[i][0] == '-' && argv[i][1] == '-') {
      fprintf (stderr, "Failed to initialize: Unknown option %s\n", argv[i]);
      return 1;
    } else if (nfiles < 2)
      files[nfiles++] = argv[i];
    else
      nfiles++;
  }
  if (gain_mode && gain_per_channel)
    gain_mode |= PEAQ_GAIN_PER_CHANNEL;
  if (bands_path && (interval_s > 0. || list_path || getenv ("PEAQ_AMD_CLI_STREAM") || getenv ("PEAQ_AMD_CLI_DUMP"))) {
    fprintf (stderr, "Failed to initialize: --bands belongs to the plain one-call mode (not with --list or --interval)\n");
    return 1;
  }
  if (bands_path && (trace_path || gain_mode || steps_window || track_window || drift_window || subsample || wide_offset)) {
    fprintf (stderr, "Failed to initialize: --bands is a run of its own (not with --trace, --match-gain or an --align-... beyond --align)\n");
    return 1;
  }
  if (bands_path && advanced && (band_planes & ~(PEAQ_BAND_NMR | PEAQ_BAND_EXC_REF))) {
    fprintf (stderr, "Failed to initialize: --bands: the advanced version has the planes nmr and exc_ref only\n");
    return 1;
  }
  if (fb_bands_path && !advanced) {
    fprintf (stderr, "Failed to initialize: --fb-bands needs --advanced (the basic version has no filter-bank path)\n");
    return 1;
  }
  if (fb_bands_path && (interval_s > 0. || list_path || getenv ("PEAQ_AMD_CLI_STREAM") || getenv ("PEAQ_AMD_CLI_DUMP"))) {
    fprintf (stderr, "Failed to initialize: --fb-bands belongs to the plain one-call mode (not with --list or --interval)\n");
    return 1;
  }
  if (fb_bands_path && (bands_path || trace_path || gain_mode || steps_window || track_window || drift_window || subsample || wide_offset)) {
    fprintf (stderr, "Failed to initialize: --fb-bands is a run of its own (not with --bands, --trace, --match-gain or an --align-... beyond --align)\n");
    return 1;
  }
  if (pattern_bands_path && advanced) {
    fprintf (stderr, "Failed to initialize: --pattern-bands covers the basic version only (with --advanced the pattern layer is the filter bank's: --fb-bands)\n");
    return 1;
  }
  if (pattern_bands_path && (interval_s > 0. || list_path || getenv ("PEAQ_AMD_CLI_STREAM") || getenv ("PEAQ_AMD_CLI_DUMP"))) {
    fprintf (stderr, "Failed to initialize: --pattern-bands belongs to the plain one-call mode (not with --list or --interval)\n");
    return 1;
  }
  if (pattern_bands_path && (bands_path || trace_path || gain_mode || steps_window || track_window || drift_window || subsample || wide_offset)) {
    fprintf (stderr, "Failed to initialize: --pattern-bands is a run of its own (not with --bands, --trace, --match-gain or an --align-... beyond --align)\n");
    return 1;
  }
  if (band_summary_path && (interval_s > 0. || list_path || getenv ("PEAQ_AMD_CLI_STREAM") || getenv ("PEAQ_AMD_CLI_DUMP"))) {
    fprintf (stderr, "Failed to initialize: --band-summary belongs to the plain one-call mode (not with --list or --interval)\n");
    return 1;
  }
  if (band_summary_path && (bands_path || fb_bands_path || pattern_bands_path || trace_path || gain_mode || steps_window || track_window || drift_window || subsample || wide_offset)) {
    fprintf (stderr, "Failed to initialize: --band-summary is a run of its own (not with --bands, --fb-bands, --pattern-bands, --trace, --match-gain or an --align-... beyond --align)\n");
    return 1;
  }
  if (fb_band_summary_path && !advanced) {
    fprintf (stderr, "Failed to initialize: --fb-band-summary needs --advanced (the basic version has no filter-bank path)\n");
    return 1;
  }
  if (fb_band_summary_path && (interval_s > 0. || list_path || getenv ("PEAQ_AMD_CLI_STREAM") || getenv ("PEAQ_AMD_CLI_DUMP"))) {
    fprintf (stderr, "Failed to initialize: --fb-band-summary belongs to the plain one-call mode (not with --list or --interval)\n");
    return 1;
  }
  if (fb_band_summary_path && (bands_path || fb_bands_path || pattern_bands_path || band_summary_path || trace_path || gain_mode || steps_window || track_window || drift_window || subsample || wide_offset)) {
    fprintf (stderr, "Failed to initialize: --fb-band-summary is a run of its own (not with --bands, --fb-bands, --pattern-bands, --band-summary, --trace, --match-gain or an --align-... beyond --align)\n");
    return 1;
  }
  if (windows_length && advanced) {
    fprintf (stderr, "Failed to initialize: --windows is for the basic version (the advanced version has --spans)\n");
    return 1;
  }
  if (spans_length && !advanced) {
    fprintf (stderr, "Failed to initialize: --spans is for the advanced version (--advanced --spans=...; the basic version has --windows)\n");
    return 1;
  }
  if (spans_length && (interval_s > 0. || list_path || getenv ("PEAQ_AMD_CLI_STREAM") || getenv ("PEAQ_AMD_CLI_DUMP"))) {
    fprintf (stderr, "Failed to initialize: --spans belongs to the plain one-call mode (not with --list or --interval)\n");
    return 1;
  }
  if (spans_length && (windows_length || bands_path || fb_bands_path || pattern_bands_path || band_summary_path || fb_band_summary_path || trace_path || gain_mode || steps_window || track_window || drift_window || subsample || wide_offset)) {
    fprintf (stderr, "Failed to initialize: --spans is a run of its own (not with --windows, --bands, --fb-bands, --pattern-bands, --band-summary, --fb-band-summary, --trace, --match-gain or an --align-... beyond --align)\n");
    return 1;
  }
  if (windows_length && (interval_s > 0. || list_path || getenv ("PEAQ_AMD_CLI_STREAM") || getenv ("PEAQ_AMD_CLI_DUMP"))) {
    fprintf (stderr, "Failed to initialize: --windows belongs to the plain one-call mode (not with --list or --interval)\n");
    return 1;
  }
  if (windows_length && (bands_path || fb_bands_path || pattern_bands_path || band_summary_path || fb_band_summary_path || trace_path || gain_mode || steps_window || track_window || drift_window || subsample || wide_offset)) {
    fprintf (stderr, "Failed to initialize: --windows is a run of its own (not with --bands, --fb-bands, --pattern-bands, --band-summary, --fb-band-summary, --trace, --match-gain or an --align-... beyond --align)\n");
    return 1;
  }
  if (gain_mode && (interval_s > 0. || trace_path || getenv ("PEAQ_AMD_CLI_STREAM") || getenv ("PEAQ_AMD_CLI_DUMP"))) {
    fprintf (stderr, "Failed to initialize: --match-gain belongs to the plain one-call mode and --list (not with --interval or --trace)\n");
    return 1;
  }
  if (wide_offset && (steps_window || track_window || drift_window || subsample)) {
    fprintf (stderr, "Failed to initialize: --align-wide is not taken with another --align-... option: their windows around a wide lag are not covered\n");
    return 1;
  }
  if (wide_offset && gain_mode) {
    fprintf (stderr, "Failed to initialize: --align-wide is not taken with --match-gain\n");
    return 1;
  }
  if (wide_offset && list_path) {
    fprintf (stderr, "Failed to initialize: --align-wide is not taken with --list: the host-fed path does not take it yet (whole-sample --align only)\n");
    return 1;
  }
  if (wide_offset && (interval_s > 0. || trace_path || getenv ("PEAQ_AMD_CLI_STREAM") || getenv ("PEAQ_AMD_CLI_DUMP"))) {
    fprintf (stderr, "Failed to initialize: --align-wide belongs to the plain one-call mode (not with --interval or --trace)\n");
    return 1;
  }
  if (steps_window && track_window) {
    fprintf (stderr, "Failed to initialize: --align-steps and --align-track exclude each other: the pieces are the track's segments, cut where a step was located\n");
    return 1;
  }
  if (steps_window && drift_window) {
    fprintf (stderr, "Failed to initialize: --align-steps and --align-drift exclude each other: the pieces are the lines, one or two per window\n");
    return 1;
  }
  if (steps_window && subsample) {
    fprintf (stderr, "Failed to initialize: --align-steps and --align-subsample exclude each other: the track's knots carry the sub-sample part\n");
    return 1;
  }
  if (steps_window && list_path) {
    fprintf (stderr, "Failed to initialize: --align-steps is not taken with --list: the host-fed path does not take it yet (whole-sample --align only)\n");
    return 1;
  }
  if (steps_window && (interval_s > 0. || trace_path || getenv ("PEAQ_AMD_CLI_STREAM") || getenv ("PEAQ_AMD_CLI_DUMP"))) {
    fprintf (stderr, "Failed to initialize: --align-steps belongs to the plain one-call mode (not with --interval or --trace)\n");
    return 1;
  }
  if (track_window && drift_window) {
    fprintf (stderr, "Failed to initialize: --align-track and --align-drift exclude each other: the track's segments are the lines, one per window\n");
    return 1;
  }
  if (track_window && subsample) {
    fprintf (stderr, "Failed to initialize: --align-track and --align-subsample exclude each other: the track's knots carry the sub-sample part\n");
    return 1;
  }
  if (track_window && list_path) {
    fprintf (stderr, "Failed to initialize: --align-track is not taken with --list: the host-fed path does not take it yet (whole-sample --align only)\n");
    return 1;
  }
  if (track_window && (interval_s > 0. || trace_path || getenv ("PEAQ_AMD_CLI_STREAM") || getenv ("PEAQ_AMD_CLI_DUMP"))) {
    fprintf (stderr, "Failed to initialize: --align-track belongs to the plain one-call mode (not with --interval or --trace)\n");
    return 1;
  }
  if (drift_window && subsample) {
    fprintf (stderr, "Failed to initialize: --align-drift and --align-subsample exclude each other: the line's offset carries the sub-sample part\n");
    return 1;
  }
  if (drift_window && list_path) {
    fprintf (stderr, "Failed to initialize: --align-drift is not taken with --list: the host-fed path does not take it yet (whole-sample --align only)\n");
    return 1;
  }
  if (drift_window && (interval_s > 0. || trace_path || getenv ("PEAQ_AMD_CLI_STREAM") || getenv ("PEAQ_AMD_CLI_DUMP"))) {
    fprintf (stderr, "Failed to initialize: --align-drift belongs to the plain one-call mode (not with --interval or --trace)\n");
    return 1;
  }
  if (subsample && list_path) {
    fprintf (stderr, "Failed to initialize: --align-subsample is not taken with --list: the host-fed path does not take it yet (whole-sample --align only)\n");
    return 1;
  }
  if (subsample && (interval_s > 0. || trace_path || getenv ("PEAQ_AMD_CLI_STREAM") || getenv ("PEAQ_AMD_CLI_DUMP"))) {
    fprintf (stderr, "Failed to initialize: --align-subsample belongs to the plain one-call mode (not with --interval or --trace)\n");
    return 1;
  }
  if (list_path) {
    if (nfiles || interval_s > 0. || trace_path) {
      fprintf (stderr, "Failed to initialize: --list takes no REFFILE TESTFILE, no --interval and no --trace\n");
      return 1;
    }
    return run_list (list_path, advanced, level, align_lag, share_refs, gain_mode, max_gain_db);
  }
  if (nfiles != 2) {
    usage (argv[0]);
    return 1;
  }
  if (trace_path && (interval_s > 0. || getenv ("PEAQ_AMD_CLI_STREAM") || getenv ("PEAQ_AMD_CLI_DUMP"))) {
    fprintf (stderr, "Failed to initialize: --trace belongs to the plain one-call mode (not with --interval)\n");
    return 1;
  }
  if (wav_read (files[0], &ref) || wav_read (files[1], &test))
    return 2;
  if (ref.rate != 48000 || test.rate != 48000) {
    if (!allow_resample || ref.rate < 8000 || test.rate < 8000) {
      fprintf (stderr, "Error: both files must be sampled at 48 kHz (got %d and %d Hz)\n", ref.rate, test.rate);
      return 2;
    }
    /* the device converter takes one rate for both signals; readings at intervals, the streaming path and the dump
     * hook work on 48 kHz samples in host memory */
    if (device_resample && !(interval_s > 0.) && !getenv ("PEAQ_AMD_CLI_STREAM") && !getenv ("PEAQ_AMD_CLI_DUMP")) {
      if (ref.rate != test.rate)
        fprintf (stderr, "Note: files at different rates (%d and %d Hz): converting on the host\n", ref.rate, test.rate);
      else if (!peaq_resample_supported ((uint32_t) ref.rate))
        fprintf (stderr, "Note: the device converter does not take %d Hz: converting on the host\n", ref.rate);
      else
        device_rate = (uint32_t) ref.rate;
    } else if (device_resample)
      fprintf (stderr, "Note: --device-resample does not apply to this mode: converting on the host\n");
    if (!device_rate && ((ref.rate != 48000 && resample_to_48k (&ref)) || (test.rate != 48000 && resample_to_48k (&test)))) {
      fprintf (stderr, "Error: out of memory while resampling\n");
      return 2;
    }
  }
  if (align_lag && (interval_s > 0. || getenv ("PEAQ_AMD_CLI_STREAM") || getenv ("PEAQ_AMD_CLI_DUMP"))) {
    fprintf (stderr, "Note: --align does not apply to this mode: comparing the files as they are\n");
    align_lag = 0;
  }
  if (ref.channels != test.channels) {
    /* the element negotiates equal channel counts via audioconvert; up-mix the mono side */
    wav_t *m = ref.channels == 1 ? &ref : &test;
    float *st = malloc ((m->frames ? m->frames : 1) * 2 * sizeof (float));
    for (pos = 0; pos < m->frames; pos++)
      st[2 * pos] = st[2 * pos + 1] = m->samples[pos];
    free (m->samples);
    m->samples = st;
    m->channels = 2;
  }
  if (getenv ("PEAQ_AMD_CLI_DUMP")) {
    /* test hook (tests/test_cli_resampler.py, runs without a GPU): what would be handed to the engine, as raw
     * interleaved F32 in <value>.ref.f32 / <value>.test.f32 -- reader, rate conversion and up-mix on their own */
    const wav_t *w[2] = { &ref, &test };
    const char *suffix[2] = { ".ref.f32", ".test.f32" };
    for (i = 0; i < 2; i++) {
      char path[4096];
      FILE *f;
      snprintf (path, sizeof path, "%s%s", getenv ("PEAQ_AMD_CLI_DUMP"), suffix[i]);
      f = fopen (path, "wb");
      if (!f || fwrite (w[i]->samples, sizeof (float), w[i]->frames * w[i]->channels, f) != w[i]->frames * w[i]->channels) {
        fprintf (stderr, "Error: cannot write %s\n", path);
        return 2;
      }
      fclose (f);
    }
    printf ("dumped %zu and %zu frames, %d channels\n", ref.frames, test.frames, ref.channels);
    return 0;
  }
  if (spans_length) {
    /* (the count print_windows is going to make, held against the limit before an engine is asked for) */
    const uint32_t rate = device_rate ? device_rate : 48000;
    const uint32_t n_r = rate == 48000 ? (uint32_t) ref.frames : peaq_resampled_length (ref.frames, rate);
    const uint32_t n_t = rate == 48000 ? (uint32_t) test.frames : peaq_resampled_length (test.frames, rate);
    const uint32_t n = n_r > n_t ? n_r : n_t;
    const size_t n_spans = 1 + (n > spans_length ? ((size_t) n - spans_length + spans_hop - 1) / spans_hop : 0);
    if (n_spans > PEAQ_WINDOWS_MAX) {
      fprintf (stderr, "Failed to initialize: --spans makes %zu spans of these files, more than %d\n", n_spans,
          PEAQ_WINDOWS_MAX);
      return 1;
    }
  }
  if (peaq_ctx_create (getenv ("PEAQ_AMD_DEVICE") ? atoi (getenv ("PEAQ_AMD_DEVICE")) : 0, &ctx) != PEAQ_OK) {
    printf ("Error: peaq engine could not be instantiated - %s\n", peaq_last_error ());
    return 2;
  }
  /* The advanced version's filter bank runs in the engine's default arithmetic, the reference's own (all FP64);
   * the faster reduced-precision bank only on request (PEAQ_AMD_FIR=f16x3, read by peaq_ctx_create). */
  if (interval_s > 0.) {
    /* readings every `interval` samples at 48 kHz (after the rate conversion) up to the end of the longer file; the
     * end result is the one of peaq_run_pair */
    const size_t n_max = ref.frames > test.frames ? ref.frames : test.frames;
    const uint32_t interval = (uint32_t) llround (interval_s * 48000.);
    const size_t n_points = n_max ? (n_max + interval - 1) / interval : 1;
    peaq_result *pts;
    size_t k;
    if (n_points > 0x7fffffff || !(pts = malloc (n_points * sizeof *pts))) {
      printf ("Error: too many readings\n");
      return 2;
    }
    if (peaq_run_pair_trajectory (ctx, advanced, ref.channels, level, ref.samples, ref.frames, test.samples,
            test.frames, interval, (int) n_points, pts, &r) != PEAQ_OK) {
      printf ("Error: %s\n", peaq_last_error ());
      return 2;
    }
    for (k = 0; k < n_points; k++) {
      const size_t end = (k + 1) * (size_t) interval < n_max ? (k + 1) * (size_t) interval : n_max;
      printf ("Time %.3f s: ODG %.3f, DI %.3f\n", end / 48000., pts[k].odg, pts[k].di);
    }
    free (pts);
  } else if (!getenv ("PEAQ_AMD_CLI_STREAM")) {
    /* both files are in memory: one call, every kernel sees the whole stream (a 5-minute pair of the advanced
     * version: 2 s instead of the 4 s of buffer-by-buffer sessions) */
    if (spans_length) {
      if (print_windows (1, spans_length, spans_hop, ctx, level, device_rate ? device_rate : 48000, align_lag, &ref, &test, &r))
        return 2;
    } else if (windows_length) {
      if (print_windows (0, windows_length, windows_hop, ctx, level, device_rate ? device_rate : 48000, align_lag, &ref, &test, &r))
        return 2;
    } else if (fb_band_summary_path) {
      if (write_fb_band_summary (fb_band_summary_path, ctx, level, device_rate ? device_rate : 48000, align_lag, &ref, &test, &r))
        return 2;
    } else if (band_summary_path) {
      if (write_band_summary (band_summary_path, ctx, advanced, level, device_rate ? device_rate : 48000, align_lag, &ref, &test, &r))
        return 2;
    } else if (pattern_bands_path) {
      if (write_band_rows (BANDS_PATTERN, pattern_bands_path, pattern_band_planes, ctx, 0, level, device_rate ? device_rate : 48000, align_lag, &ref, &test, &r))
        return 2;
    } else if (fb_bands_path) {
      if (write_band_rows (BANDS_FB, fb_bands_path, fb_band_planes, ctx, 1, level, device_rate ? device_rate : 48000, align_lag, &ref, &test, &r))
        return 2;
    } else if (bands_path) {
      if (write_band_rows (BANDS_FFT, bands_path, band_planes, ctx, advanced, level, device_rate ? device_rate : 48000, align_lag, &ref, &test, &r))
        return 2;
    } else if (trace_path) {
      if (write_trace (trace_path, ctx, advanced, level, device_rate ? device_rate : 48000, align_lag, &ref, &test, &r))
        return 2;
    } else if (steps_window) {
      char text[256];
      enum { max_steps = 64 };                          /* printed; the count of all of them is in the pieces' record */
      peaq_step found[max_steps];
      peaq_pieces pieces;
      unsigned k;
      if (peaq_run_pair_steps (ctx, advanced, ref.channels, level, device_rate ? device_rate : 48000, align_lag, steps_window,
              gain_mode, max_gain_db, ref.samples, ref.frames, test.samples, test.frames, &delay, &track, &pieces, found,
              max_steps, &gain, &r) != PEAQ_OK) {
        printf ("Error: %s\n", peaq_last_error ());
        return 2;
      }
      printf ("Delay: %d samples, track %+.4f .. %+.4f (%u of %u windows%s), %u of %u steps accepted%s\n", (int) delay.lag,
          track.d_min, track.d_max, (unsigned) track.n_valid, (unsigned) track.n_windows,
          (track.flags & PEAQ_TRACK_F_NONE) ? ", no track: no valid window" : "", (unsigned) pieces.n_accepted,
          (unsigned) pieces.n_candidates, (pieces.flags & PEAQ_PIECES_F_RANGE) ? ", slope out of range: not corrected" : "");
      for (k = 0; k < pieces.n_candidates && k < max_steps; k++)
        if (found[k].flags == 0)
          printf ("Step: at %u by %+d samples (gains %.3f and %.3f)\n", (unsigned) found[k].c, (int) (found[k].LB - found[k].LA),
              found[k].norm > 0. ? found[k].gain_left / found[k].norm : 0., found[k].norm > 0. ? found[k].gain_right / found[k].norm : 0.);
      if (gain_mode) {
        format_gain (text, sizeof text, &gain, ref.channels);
        printf ("Gain: %s\n", text);
      }
    } else if (track_window) {
      char text[256];
      if (peaq_run_pair_track (ctx, advanced, ref.channels, level, device_rate ? device_rate : 48000, align_lag, track_window,
              gain_mode, max_gain_db, ref.samples, ref.frames, test.samples, test.frames, &delay, &track, &gain, &r) != PEAQ_OK) {
        printf ("Error: %s\n", peaq_last_error ());
        return 2;
      }
      printf ("Delay: %d samples, track %+.4f .. %+.4f (%u of %u windows%s)\n", (int) delay.lag, track.d_min, track.d_max,
          (unsigned) track.n_valid, (unsigned) track.n_windows,
          (track.flags & PEAQ_TRACK_F_NONE) ? ", no track: no valid window" : (track.flags & PEAQ_TRACK_F_RANGE) ? ", slope out of range: not corrected" : "");
      if (gain_mode) {
        format_gain (text, sizeof text, &gain, ref.channels);
        printf ("Gain: %s\n", text);
      }
    } else if (drift_window) {
      char text[256];
      if (peaq_run_pair_drift (ctx, advanced, ref.channels, level, device_rate ? device_rate : 48000, align_lag, drift_window,
              gain_mode, max_gain_db, ref.samples, ref.frames, test.samples, test.frames, &delay, &drift, &gain, &r) != PEAQ_OK) {
        printf ("Error: %s\n", peaq_last_error ());
        return 2;
      }
      printf ("Delay: %d %+.4f samples, drift %+.2f ppm (%u of %u windows%s)\n", (int) delay.lag, drift.a, drift.ppm,
          (unsigned) drift.n_valid, (unsigned) drift.n_windows,
          (drift.flags & PEAQ_DRIFT_F_NONE) ? ", no line: too few valid windows" : (drift.flags & PEAQ_DRIFT_F_RANGE) ? ", slope out of range: not corrected" : "");
      if (gain_mode) {
        format_gain (text, sizeof text, &gain, ref.channels);
        printf ("Gain: %s\n", text);
      }
    } else if (subsample) {
      char text[256];
      if (peaq_run_pair_subsample (ctx, advanced, ref.channels, level, device_rate ? device_rate : 48000, align_lag, gain_mode,
              max_gain_db, ref.samples, ref.frames, test.samples, test.frames, &delay, &subdelay, &gain, &r) != PEAQ_OK) {
        printf ("Error: %s\n", peaq_last_error ());
        return 2;
      }
      printf ("Delay: %d %+.4f samples (correlation %.3f%s)\n", (int) delay.lag, subdelay.frac,
          delay.norm > 0. ? subdelay.peak / delay.norm : 0.,
          (subdelay.flags & PEAQ_SUB_F_NONE) ? ", no sub-sample estimate" : (subdelay.flags & PEAQ_SUB_F_EDGE) ? ", at the edge of the interval" : "");
      if (gain_mode) {
        format_gain (text, sizeof text, &gain, ref.channels);
        printf ("Gain: %s\n", text);
      }
    } else if (gain_mode) {
      char text[256];
      if (peaq_run_pair_matched (ctx, advanced, ref.channels, level, device_rate ? device_rate : 48000, align_lag, gain_mode,
              max_gain_db, ref.samples, ref.frames, test.samples, test.frames, &delay, &gain, &r) != PEAQ_OK) {
        printf ("Error: %s\n", peaq_last_error ());
        return 2;
      }
      if (align_lag)
        printf ("Delay: %d samples (correlation %.3f)\n", (int) delay.lag, delay.norm > 0. ? delay.peak / delay.norm : 0.);
      format_gain (text, sizeof text, &gain, ref.channels);
      printf ("Gain: %s\n", text);
    } else if (wide_offset) {
      peaq_wide_delay wide;
      if (peaq_run_pair_wide (ctx, advanced, ref.channels, level, device_rate ? device_rate : 48000, wide_offset, wide_mode,
              align_lag, ref.samples, ref.frames, test.samples, test.frames, &wide, &r) != PEAQ_OK) {
        printf ("Error: %s\n", peaq_last_error ());
        return 2;
      }
      printf ("Delay: %d samples (correlation %.3f)\n", (int) wide.lag, wide.fine.norm > 0. ? wide.fine.peak / wide.fine.norm : 0.);
      printf ("Wide: coarse %d samples, factor %u, %s (correlation %.3f)%s%s%s\n", (int) wide.coarse_lag, (unsigned) wide.factor,
          wide_mode == PEAQ_WIDE_WAVEFORM ? "waveform" : "envelope",
          wide.coarse.norm > 0. ? wide.coarse.peak / wide.coarse.norm : 0.,
          (wide.flags & PEAQ_WIDE_F_NONE) ? ", no coarse estimate" : "",
          (wide.flags & PEAQ_WIDE_F_RANGE) ? ", at the edge of the offset range" : "",
          (wide.flags & PEAQ_WIDE_F_EDGE) ? ", fine lag at the edge of its range" : "");
    } else if (align_lag) {
      if (peaq_run_pair_aligned (ctx, advanced, ref.channels, level, device_rate ? device_rate : 48000, align_lag,
              ref.samples, ref.frames, test.samples, test.frames, &delay, &r) != PEAQ_OK) {
        printf ("Error: %s\n", peaq_last_error ());
        return 2;
      }
      printf ("Delay: %d samples (correlation %.3f)\n", (int) delay.lag, delay.norm > 0. ? delay.peak / delay.norm : 0.);
    } else if ((device_rate ? peaq_run_pair_rate (ctx, advanced, ref.channels, level, device_rate, ref.samples, ref.frames,
                test.samples, test.frames, &r)
            : peaq_run_pair (ctx, advanced, ref.channels, level, ref.samples, ref.frames, test.samples, test.frames,
                &r)) != PEAQ_OK) {
      printf ("Error: %s\n", peaq_last_error ());
      return 2;
    }
  } else {
    /* PEAQ_AMD_CLI_STREAM=1: feed a session like two streaming threads would, alternating buffers of 4096
     * samples (what the `peaq` element does) */
    if (peaq_session_create (ctx, advanced, ref.channels, level, &s) != PEAQ_OK) {
      printf ("Error: peaq engine could not be instantiated - %s\n", peaq_last_error ());
      return 2;
    }
    for (pos = 0; pos < ref.frames || pos < test.frames; pos += 4096) {
      rc = PEAQ_OK;
      if (pos < ref.frames)
        rc = peaq_session_push (s, 0, ref.samples + pos * ref.channels,
            ref.frames - pos < 4096 ? ref.frames - pos : 4096);
      if (rc == PEAQ_OK && pos < test.frames)
        rc = peaq_session_push (s, 1, test.samples + pos * test.channels,
            test.frames - pos < 4096 ? test.frames - pos : 4096);
      if (rc != PEAQ_OK) {
        printf ("Error: %s\n", peaq_last_error ());
        return 2;
      }
    }
    if (peaq_session_flush (s) != PEAQ_OK || peaq_session_results (s, &r) != PEAQ_OK) {
      printf ("Error: %s\n", peaq_last_error ());
      return 2;
    }
    peaq_session_destroy (s);
  }
  printf ("Objective Difference Grade: %.3f\n", r.odg);
  printf ("Distortion Index: %.3f\n", r.di);
  peaq_ctx_destroy (ctx);
  free (ref.samples);
  free (test.samples);
  return 0;
}
