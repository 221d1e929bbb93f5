/* gstpeaq_amd.c -- the `peaq` GStreamer element on top of libpeaq_amd.so.
 *
 * Host side of the drop-in boundary: same element name, pads,
 * caps, properties, console text and flush semantics as the element of
 * HSU-ANT/gstpeaq (reference src/gstpeaq.c), but everything below the adapters
 * -- ear models, pattern processing, MOVs, accumulators, neural network -- is
 * one peaq_session of the MI355X engine (include/peaq_amd.h).
 *
 *   element "peaq", klass Sink/Audio, GST_ELEMENT_FLAG_SINK   gstpeaq.c:319-323,355
 *   sink pads "ref" and "test", ALWAYS                         gstpeaq.c:154-165
 *   caps audio/x-raw F32LE interleaved 48000 Hz                gstpeaq.c:146-152
 *   both pads negotiate the same channel count                 gstpeaq.c:216-244,689-708
 *   properties playback_level, advanced, console-output,
 *              di, odg, totalsnr                               gstpeaq.c:273-317
 *   PAUSED->READY flushes with zero padding and evaluates ODG  gstpeaq.c:764-778
 */
#include <gst/gst.h>
#include <math.h>
#include <stdio.h>
#include <string.h>

#include "peaq_amd.h"

#ifndef PACKAGE
#define PACKAGE "gstpeaq-amd"
#endif
#ifndef PACKAGE_VERSION
#define PACKAGE_VERSION "0.2.0"
#endif

GST_DEBUG_CATEGORY_STATIC (peaq_amd_debug);
#define GST_CAT_DEFAULT peaq_amd_debug

/* 48 kHz as the reference -- a structure of its own and the first, so that an upstream that can deliver 48 kHz goes on
 * doing so (audiotestsrc alone would settle on 44.1 kHz) -- and behind it the rates the device converter takes in front
 * of the model (include/peaq_amd.h, "live rate conversion"); the pads may differ */
#define PEAQ_CAPS_AT(rates) "audio/x-raw, format = (string) F32LE, layout = (string) interleaved, rate = (int) " rates
#define PEAQ_CAPS PEAQ_CAPS_AT ("48000") "; " \
    PEAQ_CAPS_AT ("{ 44100, 32000, 96000, 88200, 192000, 176400, 24000, 22050, 16000, 11025, 8000 }")

typedef struct _GstPeaqAmd
{
  GstElement element;
  GstPad *pads[2];              /* 0 = ref, 1 = test */
  gboolean eos[2];
  gboolean advanced;
  gboolean console_output;
  gdouble playback_level;
  gint channels;
  gint rate[2];                 /* what each pad's caps said; 0 until they have */
  GQueue held[2];               /* buffers that arrived before the other pad's caps: the session is made once both rates
                                 * are known, and takes them then, in order */
  guint broker_rate[2];         /* the rates the broker of this element took */
  peaq_session *session;        /* NULL until caps are known */
  peaq_broker *broker;          /* set instead of `session` when the process-wide broker serves this element */
  gint broker_sid;
  gboolean failed;              /* a device error was reported already */
  gboolean pushed;              /* the current session / broker slot has received samples */
  gchar *pending_error;         /* set under the object lock, posted after it is released */
  /* the meter (include/peaq_amd.h, "meter"): sliding-window readings of the running stream */
  gdouble meter_window, meter_hop;      /* seconds; window 0 = off, hop 0 = the window */
  guint meter_depth;
  gboolean metered;             /* the current session / broker slot has its meter on */
  gboolean meter_flushed;       /* the stream was flushed at EOS already (metered streams only) */
  gdouble st_odg, st_di, st_totalsnr;   /* the newest delivered reading, NaN before the first */
  /* live alignment (include/peaq_amd.h, "live alignment"): the chain's delay found and cut away, and watched */
  guint align_max_lag, align_probe;     /* samples at 48 kHz; max-lag 0 = no acquisition, probe 0 = the default */
  gdouble delay_watch;          /* seconds per watch window; 0 = no watch */
  gboolean aligning, watching;  /* the current session / broker slot acquires its delay / has its watch on */
  gboolean delay_acquired;      /* ... and has acquired it: `peaq-delay` has been posted */
  gint delay, delay_offset;     /* the lag acquired (0 before); the newest watch window's offset */
  gboolean watch_seen;
  guint64 watch_index;          /* the newest watch window posted */
} GstPeaqAmd;

typedef struct _GstPeaqAmdClass
{
  GstElementClass parent_class;
} GstPeaqAmdClass;

enum
{ PROP_0, PROP_PLAYBACK_LEVEL, PROP_ADVANCED, PROP_DI, PROP_ODG, PROP_TOTALSNR, PROP_CONSOLE_OUTPUT,
  PROP_METER_WINDOW, PROP_METER_HOP, PROP_METER_DEPTH, PROP_ST_ODG, PROP_ST_DI, PROP_ST_TOTALSNR,
  PROP_ALIGN_MAX_LAG, PROP_ALIGN_PROBE, PROP_DELAY_WATCH, PROP_DELAY, PROP_DELAY_ACQUIRED, PROP_DELAY_OFFSET
};

static GstStaticPadTemplate ref_template =
GST_STATIC_PAD_TEMPLATE ("ref", GST_PAD_SINK, GST_PAD_ALWAYS, GST_STATIC_CAPS (PEAQ_CAPS));
static GstStaticPadTemplate test_template =
GST_STATIC_PAD_TEMPLATE ("test", GST_PAD_SINK, GST_PAD_ALWAYS, GST_STATIC_CAPS (PEAQ_CAPS));

/* registered under the reference's type name "GstPeaq" so that unnamed instances
 * are called peaq0, peaq1, ... as before */
typedef GstPeaqAmd GstPeaq;
typedef GstPeaqAmdClass GstPeaqClass;
GType gst_peaq_amd_get_type (void);
G_DEFINE_TYPE_WITH_CODE (GstPeaq, gst_peaq_amd, GST_TYPE_ELEMENT,);
#define GST_PEAQ_AMD(obj) ((GstPeaqAmd *) (obj))

/* one device context per process */
static peaq_ctx *
shared_context (void)
{
  static gsize once = 0;
  static peaq_ctx *ctx = NULL;
  if (g_once_init_enter (&once)) {
    const gchar *dev = g_getenv ("PEAQ_AMD_DEVICE");
    if (peaq_ctx_create (dev ? atoi (dev) : 0, &ctx) != PEAQ_OK) {
      GST_ERROR ("libpeaq_amd: %s", peaq_last_error ());
      ctx = NULL;
    } else {
      /* The advanced version's filter bank runs in the engine's default arithmetic, the reference's own (all
       * FP64), whether the elements keep their own sessions or share a broker; PEAQ_AMD_FIR=f16x3 in the
       * environment selects the faster reduced-precision bank (peaq_ctx_create reads it). */
      /* decided once per process, when the first element is created: say which it was */
      GST_INFO ("libpeaq_amd: device %d, filter-bank arithmetic of the advanced version: %s", peaq_ctx_device (ctx),
                peaq_ctx_get_fir_mode (ctx) == PEAQ_FIR_F64 ? "f64" : peaq_ctx_get_fir_mode (ctx) == PEAQ_FIR_F32 ? "f32" : "f16x3");
    }
    g_once_init_leave (&once, 1);
  }
  return ctx;
}

/* PEAQ_AMD_BROKER=<max sessions>: a process that hosts many `peaq` elements lets ONE broker run
 * the frames of all of them as one batched launch per tick (include/peaq_amd.h, "broker").  One
 * broker per (version, channel count) at the default playback level; an element with another
 * level keeps its own session.  PEAQ_AMD_DEVICES=0,1,...: the broker spans those GPUs
 * (peaq_broker_create_multi: one device broker each, elements dealt out to the least loaded). */
/* PEAQ_AMD_BROKER_METER=WINDOW[:HOP] in seconds: the meter of every broker of the process (one geometry per broker,
 * because it shapes the launch).  TRUE and the values if it is set and valid. */
static gboolean
broker_meter_seconds (gdouble * window, gdouble * hop)
{
  const gchar *m = g_getenv ("PEAQ_AMD_BROKER_METER");
  gchar *end = NULL;
  if (!m || !*m)
    return FALSE;
  *window = g_ascii_strtod (m, &end);
  *hop = *window;
  if (end != m && *end == ':') {
    const gchar *h = end + 1;
    *hop = g_ascii_strtod (h, &end);
    if (end == h)
      return FALSE;
  }
  return end != m && !*end && *window > 0. && *hop > 0.;
}

static gboolean
meter_config_of (gdouble window, gdouble hop, guint depth, peaq_meter_config * cfg)
{
  cfg->depth = depth;
  return peaq_meter_frames (window, &cfg->window_frames) == PEAQ_OK
      && peaq_meter_frames (hop > 0. ? hop : window, &cfg->hop_frames) == PEAQ_OK;
}

/* max_lag, probe (samples) and the watch window (seconds) as a configuration; FALSE if the seconds are refused */
static gboolean
align_config_of (guint max_lag, guint probe, gdouble watch, peaq_live_align_config * cfg)
{
  cfg->max_lag = max_lag;
  cfg->probe = probe;
  cfg->watch_frames = cfg->reserved = 0;
  return !(watch > 0.) || peaq_meter_frames (watch, &cfg->watch_frames) == PEAQ_OK;
}

/* PEAQ_AMD_BROKER_ALIGN=MAX_LAG[:PROBE[:WATCH_SECONDS]]: the live alignment of every broker of the process (one
 * configuration per broker).  TRUE and the configuration if it is set and well-formed. */
static gboolean
broker_align_config (peaq_live_align_config * cfg)
{
  const gchar *a = g_getenv ("PEAQ_AMD_BROKER_ALIGN");
  gchar **tok;
  gboolean ok = TRUE;
  guint64 v[2] = { 0, 0 };
  gdouble watch = 0.;
  guint i, n;
  if (!a || !*a)
    return FALSE;
  tok = g_strsplit (a, ":", 4);
  n = g_strv_length (tok);
  ok = n >= 1 && n <= 3;
  for (i = 0; ok && i < n; i++) {
    gchar *end = NULL;
    if (i < 2)
      v[i] = g_ascii_strtoull (tok[i], &end, 10);
    else
      watch = g_ascii_strtod (tok[i], &end);
    ok = end != tok[i] && !*end && v[i < 2 ? i : 0] <= G_MAXUINT32 && watch >= 0.;
  }
  g_strfreev (tok);
  return ok && align_config_of ((guint) v[0], (guint) v[1], watch, cfg) && (cfg->max_lag || cfg->watch_frames);
}

/* PEAQ_AMD_BROKER_RATES=REF[:TEST] in Hz: the sampling rates of the pads of every broker of the process (one pair per
 * broker, because they size its staging); unset: 48000 on both.  FALSE if it is set and malformed. */
static gboolean
broker_rates (guint rate[2])
{
  const gchar *r = g_getenv ("PEAQ_AMD_BROKER_RATES");
  gchar *end = NULL;
  guint64 v;
  rate[0] = rate[1] = 48000;
  if (!r || !*r)
    return TRUE;
  v = g_ascii_strtoull (r, &end, 10);
  if (end == r || v > G_MAXUINT32)
    return FALSE;
  rate[0] = rate[1] = (guint) v;
  if (*end == ':') {
    const gchar *t = end + 1;
    v = g_ascii_strtoull (t, &end, 10);
    if (end == t || v > G_MAXUINT32)
      return FALSE;
    rate[1] = (guint) v;
  }
  return !*end;
}

/* taken[]: the rates the broker accepted (48000 where PEAQ_AMD_BROKER_RATES is unset, malformed or was refused) */
static peaq_broker *
shared_broker (gboolean advanced, gint channels, guint taken[2])
{
  static GMutex lock;
  static peaq_broker *brokers[2][3] = { {NULL, NULL, NULL}, {NULL, NULL, NULL} };
  static guint rates_taken[2][3][2];
  const gchar *max = g_getenv ("PEAQ_AMD_BROKER");
  const gint adv = advanced ? 1 : 0;
  peaq_broker *b = NULL;
  if (!max || atoi (max) <= 0 || channels < 1 || channels > 2)
    return NULL;
  g_mutex_lock (&lock);
  if (!brokers[adv][channels]) {
    const gchar *period = g_getenv ("PEAQ_AMD_BROKER_PERIOD_US");
    const gchar *devs = g_getenv ("PEAQ_AMD_DEVICES");
    gint devices[64], n_devices = 0, rc = PEAQ_OK;
    if (devs) {
      /* "0,1,3": device ordinals, nothing else -- a token that is not a non-negative number is an error, not device 0 */
      gchar **tok = g_strsplit (devs, ",", 64);
      for (gint i = 0; tok[i] && n_devices < 64 && rc == PEAQ_OK; i++) {
        gchar *t = g_strstrip (tok[i]), *end = NULL;
        gint64 v;
        if (!*t)
          continue;
        v = g_ascii_strtoll (t, &end, 10);
        if (end == t || *end || v < 0 || v > 1023) {
          GST_WARNING ("PEAQ_AMD_DEVICES: '%s' is not a device ordinal; no broker, one session per element", t);
          rc = PEAQ_ERR_ARG;
        } else
          devices[n_devices++] = (gint) v;
      }
      g_strfreev (tok);
    }
    if (rc != PEAQ_OK) {
      g_mutex_unlock (&lock);
      return NULL;
    }
    if (n_devices > 0) {
      /* one context per listed device inside the broker; the process-wide context of device 0 is not needed (fir_mode
       * -1: the engine's default and the environment apply to every device's context alike) */
      rc = peaq_broker_create_multi (devices, n_devices, adv, channels, 92., MAX (atoi (max), n_devices), NULL, -1,
                                     &brokers[adv][channels]);
    } else {
      peaq_ctx *ctx = shared_context ();
      rc = ctx ? peaq_broker_create (ctx, adv, channels, 92., atoi (max), &brokers[adv][channels]) : PEAQ_ERR_DEVICE;
    }
    rates_taken[adv][channels][0] = rates_taken[adv][channels][1] = 48000;
    if (rc == PEAQ_OK) {
      gdouble mw, mh;
      peaq_meter_config cfg;
      if (g_getenv ("PEAQ_AMD_BROKER_METER")) {
        if (!broker_meter_seconds (&mw, &mh) || !meter_config_of (mw, mh, 64, &cfg)
            || peaq_broker_set_meter (brokers[adv][channels], &cfg) != PEAQ_OK)
          GST_WARNING ("PEAQ_AMD_BROKER_METER: no meter (%s)", peaq_last_error ());
      }
      if (g_getenv ("PEAQ_AMD_BROKER_ALIGN")) {
        peaq_live_align_config acfg;
        if (!broker_align_config (&acfg))
          GST_WARNING ("PEAQ_AMD_BROKER_ALIGN: no alignment (not MAX_LAG[:PROBE[:WATCH_SECONDS]])");
        else if (peaq_broker_set_align (brokers[adv][channels], &acfg) != PEAQ_OK)
          GST_WARNING ("PEAQ_AMD_BROKER_ALIGN: no alignment (%s)", peaq_last_error ());
      }
      if (g_getenv ("PEAQ_AMD_BROKER_RATES")) {
        guint rates[2];
        if (!broker_rates (rates))
          GST_WARNING ("PEAQ_AMD_BROKER_RATES: 48000 Hz on both pads (not REF[:TEST])");
        else if (peaq_broker_set_rates (brokers[adv][channels], rates[0], rates[1]) != PEAQ_OK)
          GST_WARNING ("PEAQ_AMD_BROKER_RATES: 48000 Hz on both pads (%s)", peaq_last_error ());
        else {
          rates_taken[adv][channels][0] = rates[0];
          rates_taken[adv][channels][1] = rates[1];
        }
      }
      if (peaq_broker_start (brokers[adv][channels], period ? (unsigned) atoi (period) : 0) != PEAQ_OK)
        GST_WARNING ("libpeaq_amd: %s", peaq_last_error ());
    } else {
      GST_WARNING ("libpeaq_amd: no broker (%s), using one session per element", peaq_last_error ());
      brokers[adv][channels] = NULL;
    }
  }
  b = brokers[adv][channels];
  taken[0] = rates_taken[adv][channels][0];
  taken[1] = rates_taken[adv][channels][1];
  g_mutex_unlock (&lock);
  return b;
}

static void
drop_session (GstPeaqAmd * self)
{
  if (self->session)
    peaq_session_destroy (self->session);
  if (self->broker)
    peaq_broker_close (self->broker, self->broker_sid);
  self->session = NULL;
  self->broker = NULL;
}

/* (re)create the engine session: the reference re-allocates all per-channel state
 * whenever caps or the `advanced` property change (gstpeaq.c:519,559,575,586).
 * Called with the object lock held: a failure is only RECORDED here
 * (pending_error); GST_ELEMENT_ERROR takes the same non-recursive lock, so the
 * callers post it through post_pending_error() after unlocking. */
static gboolean
renew_session (GstPeaqAmd * self)
{
  peaq_ctx *ctx;
  drop_session (self);
  self->pushed = FALSE;
  self->metered = self->meter_flushed = FALSE;
  self->st_odg = self->st_di = self->st_totalsnr = NAN;
  self->aligning = self->watching = self->delay_acquired = self->watch_seen = FALSE;
  self->delay = self->delay_offset = 0;
  /* (not before both pads' rates are known: what a pad pushes until then waits in `held`) */
  if (self->channels <= 0 || !self->rate[0] || !self->rate[1])
    return TRUE;
  if (self->playback_level == 92.) {
    peaq_broker *b = shared_broker (self->advanced, self->channels, self->broker_rate);
    if (b && peaq_broker_open (b, &self->broker_sid) == PEAQ_OK) {
      gdouble mw, mh;
      peaq_live_align_config acfg;
      self->broker = b;
      self->metered = broker_meter_seconds (&mw, &mh);    /* the geometry is the process's, not the element's */
      if (broker_align_config (&acfg)) {                /* ... and so is the alignment */
        self->aligning = acfg.max_lag != 0;
        self->watching = acfg.watch_frames != 0;
      }
      return TRUE;
    }
  }
  ctx = shared_context ();
  if (!ctx || peaq_session_create (ctx, self->advanced, self->channels, self->playback_level,
          &self->session) != PEAQ_OK) {
    g_free (self->pending_error);
    self->pending_error = g_strdup_printf ("libpeaq_amd: %s", peaq_last_error ());
    self->session = NULL;
    return FALSE;
  }
  if ((self->rate[0] != 48000 || self->rate[1] != 48000)
      && peaq_session_set_rates (self->session, (guint) self->rate[0], (guint) self->rate[1]) != PEAQ_OK) {
    g_free (self->pending_error);
    self->pending_error = g_strdup_printf ("libpeaq_amd: %s", peaq_last_error ());
    drop_session (self);
    return FALSE;
  }
  if (self->meter_window > 0.) {
    peaq_meter_config cfg;
    if (meter_config_of (self->meter_window, self->meter_hop, self->meter_depth, &cfg)
        && peaq_session_set_meter (self->session, &cfg) == PEAQ_OK)
      self->metered = TRUE;
    else
      GST_WARNING_OBJECT (self, "libpeaq_amd: no meter (%s)", peaq_last_error ());
  }
  if (self->align_max_lag || self->delay_watch > 0.) {
    peaq_live_align_config cfg;
    if (align_config_of (self->align_max_lag, self->align_probe, self->delay_watch, &cfg)
        && peaq_session_set_align (self->session, &cfg) == PEAQ_OK) {
      self->aligning = cfg.max_lag != 0;
      self->watching = cfg.watch_frames != 0;
    } else
      GST_WARNING_OBJECT (self, "libpeaq_amd: no alignment (%s)", peaq_last_error ());
  }
  return TRUE;
}

/* Live alignment on the bus: once, when the stream's delay has been acquired, an element message `peaq-delay` (lag,
 * peak, runner-up, norm, skip-ref, skip-test); for every new watch window an element message `peaq-delay-watch` (index,
 * first-frame, frames, offset, peak, runner-up, norm).  Call WITHOUT the object lock (posting takes it). */
static void
post_alignment (GstPeaqAmd * self)
{
  peaq_live_delay d;
  peaq_delay_watch w;
  gboolean new_delay = FALSE, new_window = FALSE;
  GST_OBJECT_LOCK (self);
  if (self->aligning && !self->delay_acquired) {
    gint rc = self->broker ? peaq_broker_align_read (self->broker, self->broker_sid, &d)
        : self->session ? peaq_session_align_read (self->session, &d) : PEAQ_ERR_ARG;
    if (rc == PEAQ_OK && d.acquired) {
      self->delay_acquired = new_delay = TRUE;
      self->delay = d.d.lag;
    }
  }
  if (self->watching) {
    gint rc = self->broker ? peaq_broker_watch_read (self->broker, self->broker_sid, &w)
        : self->session ? peaq_session_watch_read (self->session, &w) : PEAQ_ERR_ARG;
    if (rc == PEAQ_OK && w.n_frames && (!self->watch_seen || w.index != self->watch_index)) {
      self->watch_seen = new_window = TRUE;
      self->watch_index = w.index;
      self->delay_offset = w.offset;
    }
  }
  GST_OBJECT_UNLOCK (self);
  if (new_delay) {
    g_object_notify (G_OBJECT (self), "delay");
    g_object_notify (G_OBJECT (self), "delay-acquired");
  }
  if (new_window)
    g_object_notify (G_OBJECT (self), "delay-offset");
  if (new_delay)
    gst_element_post_message (GST_ELEMENT (self), gst_message_new_element (GST_OBJECT (self),
            gst_structure_new ("peaq-delay", "lag", G_TYPE_INT, (gint) d.d.lag, "peak", G_TYPE_DOUBLE, d.d.peak,
                "runner-up", G_TYPE_DOUBLE, d.d.runner_up, "norm", G_TYPE_DOUBLE, d.d.norm,
                "skip-ref", G_TYPE_UINT, (guint) d.skip_ref, "skip-test", G_TYPE_UINT, (guint) d.skip_test, NULL)));
  if (new_window)
    gst_element_post_message (GST_ELEMENT (self), gst_message_new_element (GST_OBJECT (self),
            gst_structure_new ("peaq-delay-watch", "index", G_TYPE_UINT64, (guint64) w.index,
                "first-frame", G_TYPE_UINT, (guint) w.first_frame, "frames", G_TYPE_UINT, (guint) w.n_frames,
                "offset", G_TYPE_INT, (gint) w.offset, "peak", G_TYPE_DOUBLE, w.peak, "runner-up", G_TYPE_DOUBLE,
                w.runner_up, "norm", G_TYPE_DOUBLE, w.norm, NULL)));
}

/* The readings delivered since the last call, each as an element message `peaq-meter` on the bus: index, start and
 * duration (clock times of the window's first sample and of its samples, frames of 2048 every 1024 at 48 kHz), odg,
 * di, totalsnr, movs.  Call WITHOUT the object lock (posting takes it). */
static void
post_meter_readings (GstPeaqAmd * self)
{
  for (;;) {
    peaq_meter_reading rows[16];
    gint n = 0, i, rc;
    gboolean adv;
    GST_OBJECT_LOCK (self);
    adv = self->advanced;
    if (!self->metered)
      rc = PEAQ_ERR_ARG;
    else if (self->broker)
      rc = peaq_broker_meter_read (self->broker, self->broker_sid, rows, 16, &n, NULL);
    else if (self->session)
      rc = peaq_session_meter_read (self->session, rows, 16, &n, NULL);
    else
      rc = PEAQ_ERR_ARG;
    if (rc == PEAQ_OK && n > 0) {
      self->st_odg = rows[n - 1].r.odg;
      self->st_di = rows[n - 1].r.di;
      self->st_totalsnr = rows[n - 1].r.totalsnr;
    }
    GST_OBJECT_UNLOCK (self);
    if (rc != PEAQ_OK || n <= 0)
      return;
    for (i = 0; i < n; i++) {
      const peaq_meter_reading *m = &rows[i];
      GValue movs = G_VALUE_INIT;
      GstStructure *st;
      gint k;
      g_value_init (&movs, GST_TYPE_ARRAY);
      for (k = 0; k < (adv ? PEAQ_MOVS_ADVANCED : PEAQ_MOVS_BASIC); k++) {
        GValue v = G_VALUE_INIT;
        g_value_init (&v, G_TYPE_DOUBLE);
        g_value_set_double (&v, m->r.movs[k]);
        gst_value_array_append_value (&movs, &v);
        g_value_unset (&v);
      }
      st = gst_structure_new ("peaq-meter", "index", G_TYPE_UINT64, (guint64) m->index,
          "start", GST_TYPE_CLOCK_TIME, gst_util_uint64_scale ((guint64) m->first_frame * 1024, GST_SECOND, 48000),
          "duration", GST_TYPE_CLOCK_TIME, gst_util_uint64_scale (((guint64) m->n_frames + 1) * 1024, GST_SECOND, 48000),
          "odg", G_TYPE_DOUBLE, m->r.odg, "di", G_TYPE_DOUBLE, m->r.di, "totalsnr", G_TYPE_DOUBLE, m->r.totalsnr, NULL);
      gst_structure_take_value (st, "movs", &movs);
      gst_element_post_message (GST_ELEMENT (self), gst_message_new_element (GST_OBJECT (self), st));
    }
    if (n < 16)
      return;
  }
}

/* call WITHOUT the object lock */
static void
post_pending_error (GstPeaqAmd * self)
{
  gchar *msg;
  GST_OBJECT_LOCK (self);
  msg = self->pending_error;
  self->pending_error = NULL;
  GST_OBJECT_UNLOCK (self);
  if (msg) {
    GST_ELEMENT_ERROR (self, LIBRARY, INIT, ("%s", msg), (NULL));
    g_free (msg);
  }
}

static gboolean
read_results (GstPeaqAmd * self, peaq_result * r)
{
  if (self->broker && peaq_broker_results (self->broker, self->broker_sid, r) == PEAQ_OK)
    return TRUE;
  if (!self->session || peaq_session_results (self->session, r) != PEAQ_OK) {
    gint i;
    for (i = 0; i < PEAQ_MOVS_BASIC; i++)
      r->movs[i] = NAN;
    r->di = r->odg = r->totalsnr = NAN;      /* no data yet: the reference's empty accumulators give NaN too */
    return FALSE;
  }
  return TRUE;
}

/* console text of the reference, gstpeaq.c:1023-1035,1051-1060,1075 */
static void
print_movs (const GstPeaqAmd * self, const peaq_result * r)
{
  const gdouble *m = r->movs;
  if (!self->console_output)
    return;
  if (self->advanced)
    g_print ("RmsModDiffA = %f\nRmsNoiseLoudAsymA = %f\nSegmentalNMRB = %f\nEHSB = %f\nAvgLinDistA = %f\n",
        m[0], m[1], m[2], m[3], m[4]);
  else
    g_print ("   BandwidthRefB: %f\n  BandwidthTestB: %f\n      Total NMRB: %f\n"
        "    WinModDiff1B: %f\n            ADBB: %f\n            EHSB: %f\n"
        "    AvgModDiff1B: %f\n    AvgModDiff2B: %f\n   RmsNoiseLoudB: %f\n"
        "           MFPDB: %f\n  RelDistFramesB: %f\n",
        m[0], m[1], m[2], m[3], m[4], m[5], m[6], m[7], m[8], m[9], m[10]);
}

static gdouble
evaluate_odg (GstPeaqAmd * self)
{
  peaq_result r;
  read_results (self, &r);
  print_movs (self, &r);
  if (self->console_output)
    g_print ("Objective Difference Grade: %.3f\n", r.odg);
  return r.odg;
}

static void
gst_peaq_amd_get_property (GObject * obj, guint id, GValue * value, GParamSpec * pspec)
{
  GstPeaqAmd *self = GST_PEAQ_AMD (obj);
  peaq_result r;
  switch (id) {
    case PROP_PLAYBACK_LEVEL:
      g_value_set_double (value, self->playback_level);
      break;
    case PROP_ADVANCED:
      g_value_set_boolean (value, self->advanced);
      break;
    case PROP_CONSOLE_OUTPUT:
      g_value_set_boolean (value, self->console_output);
      break;
    case PROP_DI:
      read_results (self, &r);
      print_movs (self, &r);
      g_value_set_double (value, r.di);
      break;
    case PROP_ODG:
      g_value_set_double (value, evaluate_odg (self));
      break;
    case PROP_TOTALSNR:
      read_results (self, &r);
      g_value_set_double (value, r.totalsnr);
      break;
    case PROP_METER_WINDOW:
    case PROP_METER_HOP:{
      /* an element hosted by the broker reads back the broker's values */
      gdouble w = self->meter_window, h = self->meter_hop > 0. ? self->meter_hop : self->meter_window, bw, bh;
      if (self->broker && broker_meter_seconds (&bw, &bh)) {
        w = bw;
        h = bh;
      }
      g_value_set_double (value, id == PROP_METER_WINDOW ? w : h);
      break;
    }
    case PROP_METER_DEPTH:
      g_value_set_uint (value, self->broker ? 64 : self->meter_depth);
      break;
    case PROP_ST_ODG:
      g_value_set_double (value, self->st_odg);
      break;
    case PROP_ST_DI:
      g_value_set_double (value, self->st_di);
      break;
    case PROP_ST_TOTALSNR:
      g_value_set_double (value, self->st_totalsnr);
      break;
    case PROP_ALIGN_MAX_LAG:
    case PROP_ALIGN_PROBE:
    case PROP_DELAY_WATCH:{
      /* an element hosted by the broker reads back the broker's values (the watch window rounded to frames) */
      peaq_live_align_config b = { self->align_max_lag, self->align_probe, 0, 0 };
      gdouble watch = self->delay_watch;
      if (self->broker && broker_align_config (&b))
        watch = b.watch_frames * 1024. / 48000.;
      else if (self->broker)
        b.max_lag = b.probe = 0, watch = 0.;
      if (id == PROP_DELAY_WATCH)
        g_value_set_double (value, watch);
      else
        g_value_set_uint (value, id == PROP_ALIGN_MAX_LAG ? b.max_lag : b.probe);
      break;
    }
    case PROP_DELAY:
      g_value_set_int (value, self->delay);
      break;
    case PROP_DELAY_ACQUIRED:
      g_value_set_boolean (value, self->delay_acquired);
      break;
    case PROP_DELAY_OFFSET:
      g_value_set_int (value, self->delay_offset);
      break;
    default:
      G_OBJECT_WARN_INVALID_PROPERTY_ID (obj, id, pspec);
  }
}

static void
gst_peaq_amd_set_property (GObject * obj, guint id, const GValue * value, GParamSpec * pspec)
{
  GstPeaqAmd *self = GST_PEAQ_AMD (obj);
  switch (id) {
    case PROP_PLAYBACK_LEVEL:
      GST_OBJECT_LOCK (self);
      self->playback_level = g_value_get_double (value);
      /* the reference hands the level to both ear models at once (gstpeaq.c:508-515 ->
       * fftearmodel.c:305-314, fbearmodel.c:249-254): it applies from the next frame on */
      if (self->session) {
        if (peaq_session_set_level (self->session, self->playback_level) != PEAQ_OK)
          GST_WARNING_OBJECT (self, "libpeaq_amd: %s", peaq_last_error ());
      } else if (self->broker && self->playback_level != 92.) {
        /* the shared broker runs all its slots at one level: an element that wants another
         * one gets its own session -- possible as long as its slot has not seen any samples */
        if (!self->pushed)
          renew_session (self);
        else
          GST_WARNING_OBJECT (self, "playback_level changed mid-stream on a broker-hosted element: "
              "the new level applies from the next (re)negotiation");
      }
      GST_OBJECT_UNLOCK (self);
      post_pending_error (self);
      break;
    case PROP_ADVANCED:
      GST_OBJECT_LOCK (self);
      self->advanced = g_value_get_boolean (value);
      if (self->channels > 0)
        renew_session (self);
      GST_OBJECT_UNLOCK (self);
      post_pending_error (self);
      break;
    case PROP_CONSOLE_OUTPUT:
      self->console_output = g_value_get_boolean (value);
      break;
    case PROP_METER_WINDOW:
    case PROP_METER_HOP:
    case PROP_METER_DEPTH:
      /* like `advanced`: in NULL / READY; the session is made anew if there is one and it has seen no samples */
      GST_OBJECT_LOCK (self);
      if (id == PROP_METER_WINDOW)
        self->meter_window = g_value_get_double (value);
      else if (id == PROP_METER_HOP)
        self->meter_hop = g_value_get_double (value);
      else
        self->meter_depth = g_value_get_uint (value);
      if (self->channels > 0 && !self->pushed)
        renew_session (self);
      else if (self->pushed)
        GST_WARNING_OBJECT (self, "the meter's geometry changed mid-stream: it applies from the next (re)negotiation");
      GST_OBJECT_UNLOCK (self);
      post_pending_error (self);
      break;
    case PROP_ALIGN_MAX_LAG:
    case PROP_ALIGN_PROBE:
    case PROP_DELAY_WATCH:
      /* like the meter's: in NULL / READY; the session is made anew if there is one and it has seen no samples */
      GST_OBJECT_LOCK (self);
      if (id == PROP_ALIGN_MAX_LAG)
        self->align_max_lag = g_value_get_uint (value);
      else if (id == PROP_ALIGN_PROBE)
        self->align_probe = g_value_get_uint (value);
      else
        self->delay_watch = g_value_get_double (value);
      if (self->channels > 0 && !self->pushed)
        renew_session (self);
      else if (self->pushed)
        GST_WARNING_OBJECT (self, "the alignment changed mid-stream: it applies from the next (re)negotiation");
      GST_OBJECT_UNLOCK (self);
      post_pending_error (self);
      break;
    default:
      G_OBJECT_WARN_INVALID_PROPERTY_ID (obj, id, pspec);
  }
}

static gint
pad_index (GstPeaqAmd * self, GstPad * pad)
{
  return pad == self->pads[0] ? 0 : 1;
}

/* samples into the session or the broker slot (the caller holds the object lock) */
static GstFlowReturn
push_samples (GstPeaqAmd * self, gint idx, const guint8 * data, gsize size)
{
  const size_t n = size / (sizeof (float) * self->channels);
  if (self->broker)
    return peaq_broker_push (self->broker, self->broker_sid, idx, (const float *) data, n) == PEAQ_OK ? GST_FLOW_OK : GST_FLOW_ERROR;
  if (!self->session)
    return GST_FLOW_NOT_NEGOTIATED;
  return peaq_session_push (self->session, idx, (const float *) data, n) == PEAQ_OK ? GST_FLOW_OK : GST_FLOW_ERROR;
}

/* what the pads pushed before the session existed, in order (the caller holds the object lock); FALSE: a push failed */
static gboolean
push_held (GstPeaqAmd * self)
{
  gboolean ok = TRUE;
  gint idx;
  for (idx = 0; idx < 2; idx++) {
    GstBuffer *b;
    while ((b = g_queue_pop_head (&self->held[idx]))) {
      GstMapInfo map;
      if (ok && (self->session || self->broker) && gst_buffer_map (b, &map, GST_MAP_READ)) {
        ok = push_samples (self, idx, map.data, map.size) == GST_FLOW_OK;
        gst_buffer_unmap (b, &map);
      }
      gst_buffer_unref (b);
    }
  }
  return ok;
}

/* A stream ends (or the element stops) while one pad never had caps: that pad counts as 48 kHz, and the session is made
 * for what the other one pushed (the caller holds the object lock). */
static void
settle_unknown_rates (GstPeaqAmd * self)
{
  if (self->session || self->broker || self->channels <= 0 || !(self->rate[0] || self->rate[1]))
    return;
  if (!self->rate[0])
    self->rate[0] = 48000;
  if (!self->rate[1])
    self->rate[1] = 48000;
  if (renew_session (self) && !push_held (self))
    GST_ERROR_OBJECT (self, "libpeaq_amd: %s", peaq_last_error ());
}

static GstFlowReturn
gst_peaq_amd_chain (GstPad * pad, GstObject * parent, GstBuffer * buffer)
{
  GstPeaqAmd *self = GST_PEAQ_AMD (parent);
  GstMapInfo map;
  GstFlowReturn ret = GST_FLOW_OK;
  const gint idx = pad_index (self, pad);

  if (!gst_buffer_map (buffer, &map, GST_MAP_READ)) {
    gst_buffer_unref (buffer);
    return GST_FLOW_ERROR;
  }
  GST_OBJECT_LOCK (self);               /* the two streaming threads are serialised, gstpeaq.c:619,658 */
  self->eos[idx] = FALSE;
  self->pushed = TRUE;
  if (!self->session && !self->broker && self->rate[idx] && !self->rate[1 - idx]) {
    /* this pad has its caps, the other one not yet: the buffer waits for the session */
    g_queue_push_tail (&self->held[idx], gst_buffer_ref (buffer));
  } else
    ret = push_samples (self, idx, map.data, map.size);
  GST_OBJECT_UNLOCK (self);
  if (ret == GST_FLOW_OK && self->metered)
    post_meter_readings (self);         /* what this push completed (a broker: what its ticks have delivered so far) */
  if (ret == GST_FLOW_OK && (self->aligning || self->watching))
    post_alignment (self);
  if (ret == GST_FLOW_ERROR && !self->failed) {
    self->failed = TRUE;
    GST_ELEMENT_ERROR (self, LIBRARY, FAILED, ("libpeaq_amd: %s", peaq_last_error ()), (NULL));
  }
  gst_buffer_unmap (buffer, &map);
  gst_buffer_unref (buffer);           /* the samples were copied by the engine */
  return ret;
}

static gboolean
gst_peaq_amd_set_caps (GstPeaqAmd * self, gint idx, GstCaps * caps)
{
  gint channels = 0, rate = 48000;
  gboolean ok = TRUE;
  if (!gst_structure_get_int (gst_caps_get_structure (caps, 0), "channels", &channels) || channels < 1
      || channels > 2) {
    GST_ELEMENT_ERROR (self, CORE, NEGOTIATION, ("peaq handles mono or stereo, got %d channels", channels), (NULL));
    return FALSE;
  }
  if (!gst_structure_get_int (gst_caps_get_structure (caps, 0), "rate", &rate) || rate <= 0)
    rate = 48000;
  GST_OBJECT_LOCK (self);
  /* Both pads' rates go to the session, so it is made when the second pad's caps are known; what the first pad pushed
   * until then was held back and goes in now.  Later caps: a new session where the channels or, in mid-stream, a rate
   * changed -- as the reference re-allocates on new caps --, else the one that is there, whose stream has not begun. */
  if (channels != self->channels || !(self->session || self->broker) || (rate != self->rate[idx] && self->pushed)) {
    const gboolean restart = (self->session || self->broker) || (self->channels > 0 && channels != self->channels);
    if (restart) {                      /* (a stream of other channels or another rate: nothing held belongs to it) */
      gint i;
      for (i = 0; i < 2; i++)
        g_queue_clear_full (&self->held[i], (GDestroyNotify) gst_buffer_unref);
    }
    self->channels = channels;
    self->rate[idx] = rate;
    ok = renew_session (self);
    if (ok && (self->session || self->broker) && !push_held (self)) {
      g_free (self->pending_error);
      self->pending_error = g_strdup_printf ("libpeaq_amd: %s", peaq_last_error ());
      ok = FALSE;
    }
  } else if (rate != self->rate[idx]) {
    self->rate[idx] = rate;
    if (self->session && peaq_session_set_rates (self->session, (guint) self->rate[0], (guint) self->rate[1]) != PEAQ_OK) {
      g_free (self->pending_error);
      self->pending_error = g_strdup_printf ("libpeaq_amd: %s", peaq_last_error ());
      ok = FALSE;
    }
  }
  /* a broker's rates are the process's (PEAQ_AMD_BROKER_RATES, as far as the broker took them): a pad with another
   * rate cannot ride in it */
  if (ok && self->broker) {
    gint i;
    for (i = 0; i < 2 && ok; i++)
      if (self->broker_rate[i] != (guint) self->rate[i]) {
        g_free (self->pending_error);
        self->pending_error =
            g_strdup_printf ("peaq: the %s pad's caps say %d Hz, the broker of this process takes %u Hz there "
            "(PEAQ_AMD_BROKER_RATES=REF[:TEST])", i ? "test" : "ref", self->rate[i], self->broker_rate[i]);
        ok = FALSE;
      }
  }
  GST_OBJECT_UNLOCK (self);
  post_pending_error (self);
  return ok;
}

/* a copy of caps without the rates: the pads agree on channels and format, not on the rate */
static GstCaps *
caps_without_rate (GstCaps * caps)
{
  GstCaps *c = gst_caps_copy (caps);
  guint i;
  for (i = 0; i < gst_caps_get_size (c); i++)
    gst_structure_remove_field (gst_caps_get_structure (c, i), "rate");
  return c;
}

static gboolean
gst_peaq_amd_sink_event (GstPad * pad, GstObject * parent, GstEvent * event)
{
  GstPeaqAmd *self = GST_PEAQ_AMD (parent);
  const gint idx = pad_index (self, pad);
  gboolean ret;
  switch (GST_EVENT_TYPE (event)) {
    case GST_EVENT_EOS:{
      /* a sink posts EOS once ALL its pads are at EOS (gstpeaq.c:668-688).  Under the object lock: the two pads'
       * streaming threads get here at the same moment often enough (one process in thirty with 1024 elements), and
       * unlocked each could write its own flag, read the other's old value and leave the posting to the other --
       * a pipeline that never ends. */
      gboolean both;
      GST_OBJECT_LOCK (self);
      self->eos[idx] = TRUE;
      both = self->eos[0] && self->eos[1];
      if (both)
        settle_unknown_rates (self);
      GST_OBJECT_UNLOCK (self);
      ret = TRUE;
      if (both && (self->metered || self->aligning || self->watching)) {
        /* a metered, aligned or watched stream is flushed here, not at PAUSED -> READY, so that its last readings (and
         * the delay of a stream that ended before its probe was full) are on the bus before the EOS message; the
         * flush at the state change then finds nothing left, and the results are the same */
        peaq_result r;
        GST_OBJECT_LOCK (self);
        if (!self->meter_flushed) {
          self->meter_flushed = TRUE;
          if ((self->broker && (peaq_broker_flush (self->broker, self->broker_sid) != PEAQ_OK
                      || peaq_broker_results (self->broker, self->broker_sid, &r) != PEAQ_OK))
              || (self->session && peaq_session_flush (self->session) != PEAQ_OK))
            GST_ERROR_OBJECT (self, "libpeaq_amd: %s", peaq_last_error ());
        }
        GST_OBJECT_UNLOCK (self);
        post_meter_readings (self);
        post_alignment (self);
      }
      if (both) {
        GstMessage *msg = gst_message_new_eos (parent);
        gst_message_set_seqnum (msg, gst_event_get_seqnum (event));
        ret = gst_element_post_message (GST_ELEMENT (self), msg);
      }
      gst_event_unref (event);
      return ret;
    }
    case GST_EVENT_CAPS:{
      GstCaps *caps;
      gst_event_parse_caps (event, &caps);
      /* both inputs must carry the same number of channels: only accept what the
       * other pad's upstream can also deliver (gstpeaq.c:689-708) */
      {
        /* (the rate aside: a fixed rate of its own is the other pad's business) */
        GstCaps *other = gst_pad_peer_query_caps (self->pads[1 - idx], NULL), *mine = caps_without_rate (caps);
        GstCaps *theirs = caps_without_rate (other);
        ret = gst_caps_can_intersect (mine, theirs) && gst_peaq_amd_set_caps (self, idx, caps);
        gst_caps_unref (other);
        gst_caps_unref (mine);
        gst_caps_unref (theirs);
      }
      gst_event_unref (event);
      return ret;
    }
    default:
      return gst_pad_event_default (pad, parent, event);
  }
}

static gboolean
gst_peaq_amd_sink_query (GstPad * pad, GstObject * parent, GstQuery * query)
{
  GstPeaqAmd *self = GST_PEAQ_AMD (parent);
  if (GST_QUERY_TYPE (query) == GST_QUERY_CAPS) {
    /* offer the template caps restricted to what the OTHER input can produce */
    const gint idx = pad_index (self, pad);
    GstCaps *filter, *tmpl, *other, *any_rate, *result;
    gst_query_parse_caps (query, &filter);
    tmpl = gst_pad_get_pad_template_caps (pad);
    if (filter) {
      GstCaps *f = caps_without_rate (filter);
      other = gst_pad_peer_query_caps (self->pads[1 - idx], f);
      gst_caps_unref (f);
    } else
      other = gst_pad_peer_query_caps (self->pads[1 - idx], NULL);
    any_rate = caps_without_rate (other);           /* (each pad keeps the rate of its own upstream) */
    result = gst_caps_intersect_full (tmpl, any_rate, GST_CAPS_INTERSECT_FIRST);   /* (48 kHz stays first) */
    gst_caps_unref (any_rate);
    gst_caps_unref (tmpl);
    gst_caps_unref (other);
    gst_query_set_caps_result (query, result);
    gst_caps_unref (result);
    return TRUE;
  }
  return gst_pad_query_default (pad, parent, query);
}

static GstStateChangeReturn
gst_peaq_amd_change_state (GstElement * element, GstStateChange transition)
{
  GstPeaqAmd *self = GST_PEAQ_AMD (element);
  if (transition == GST_STATE_CHANGE_PAUSED_TO_READY) {
    /* do_flush + calculate_odg, gstpeaq.c:764-778 */
    GST_OBJECT_LOCK (self);
    settle_unknown_rates (self);
    GST_OBJECT_UNLOCK (self);
    if ((self->broker && peaq_broker_flush (self->broker, self->broker_sid) != PEAQ_OK)
        || (self->session && peaq_session_flush (self->session) != PEAQ_OK))
      GST_ERROR_OBJECT (self, "libpeaq_amd: %s", peaq_last_error ());
    evaluate_odg (self);
  }
  return GST_ELEMENT_CLASS (gst_peaq_amd_parent_class)->change_state (element, transition);
}

static void
gst_peaq_amd_finalize (GObject * obj)
{
  GstPeaqAmd *self = GST_PEAQ_AMD (obj);
  drop_session (self);
  g_queue_clear_full (&self->held[0], (GDestroyNotify) gst_buffer_unref);
  g_queue_clear_full (&self->held[1], (GDestroyNotify) gst_buffer_unref);
  g_free (self->pending_error);
  G_OBJECT_CLASS (gst_peaq_amd_parent_class)->finalize (obj);
}

static void
gst_peaq_amd_class_init (GstPeaqAmdClass * klass)
{
  GObjectClass *oc = G_OBJECT_CLASS (klass);
  GstElementClass *ec = GST_ELEMENT_CLASS (klass);

  oc->get_property = gst_peaq_amd_get_property;
  oc->set_property = gst_peaq_amd_set_property;
  oc->finalize = gst_peaq_amd_finalize;
  ec->change_state = gst_peaq_amd_change_state;

  /* names, ranges and defaults as in gstpeaq.c:273-317 ("playback_level" with an underscore) */
  g_object_class_install_property (oc, PROP_PLAYBACK_LEVEL,
      g_param_spec_double ("playback_level", "playback level", "Playback level in dB", 0, 130, 92,
          G_PARAM_READWRITE | G_PARAM_CONSTRUCT));
  g_object_class_install_property (oc, PROP_ADVANCED,
      g_param_spec_boolean ("advanced", "Advanced mode enabled", "True if advanced mode is used", FALSE,
          G_PARAM_READWRITE | G_PARAM_CONSTRUCT));
  g_object_class_install_property (oc, PROP_DI,
      g_param_spec_double ("di", "distortion index", "Distortion Index", -G_MAXDOUBLE, G_MAXDOUBLE, 0,
          G_PARAM_READABLE));
  g_object_class_install_property (oc, PROP_ODG,
      g_param_spec_double ("odg", "objective difference grade", "Objective Difference Grade", -G_MAXDOUBLE,
          G_MAXDOUBLE, 0, G_PARAM_READABLE));
  g_object_class_install_property (oc, PROP_TOTALSNR,
      g_param_spec_double ("totalsnr", "the overall SNR in dB", "the overall signal to noise ratio in dB",
          -G_MAXDOUBLE, G_MAXDOUBLE, 0, G_PARAM_READABLE));
  g_object_class_install_property (oc, PROP_CONSOLE_OUTPUT,
      g_param_spec_boolean ("console-output", "console output", "Enable or disable console output", TRUE,
          G_PARAM_READWRITE | G_PARAM_CONSTRUCT));

  /* the meter: sliding-window readings of the running stream (include/peaq_amd.h, "meter") */
  g_object_class_install_property (oc, PROP_METER_WINDOW,
      g_param_spec_double ("meter-window", "meter window", "Length of the meter's window in seconds (0 = off)", 0, 1e6, 0,
          G_PARAM_READWRITE | G_PARAM_CONSTRUCT));
  g_object_class_install_property (oc, PROP_METER_HOP,
      g_param_spec_double ("meter-hop", "meter hop", "Seconds between the meter's windows (0 = the window)", 0, 1e6, 0,
          G_PARAM_READWRITE | G_PARAM_CONSTRUCT));
  g_object_class_install_property (oc, PROP_METER_DEPTH,
      g_param_spec_uint ("meter-depth", "meter depth", "Readings the meter keeps for a reader that falls behind", 1, 4096,
          64, G_PARAM_READWRITE | G_PARAM_CONSTRUCT));
  g_object_class_install_property (oc, PROP_ST_ODG,
      g_param_spec_double ("short-term-odg", "short-term ODG", "ODG of the newest window of the meter (NaN before the first)",
          -G_MAXDOUBLE, G_MAXDOUBLE, 0, G_PARAM_READABLE));
  g_object_class_install_property (oc, PROP_ST_DI,
      g_param_spec_double ("short-term-di", "short-term DI", "Distortion index of the newest window of the meter",
          -G_MAXDOUBLE, G_MAXDOUBLE, 0, G_PARAM_READABLE));
  g_object_class_install_property (oc, PROP_ST_TOTALSNR,
      g_param_spec_double ("short-term-totalsnr", "short-term SNR", "Overall SNR in dB of the newest window of the meter",
          -G_MAXDOUBLE, G_MAXDOUBLE, 0, G_PARAM_READABLE));

  /* live alignment: the chain's delay found and cut away, and watched (include/peaq_amd.h, "live alignment") */
  g_object_class_install_property (oc, PROP_ALIGN_MAX_LAG,
      g_param_spec_uint ("align-max-lag", "alignment search range",
          "Largest delay between the pads searched for, in samples at 48 kHz (0 = no alignment)", 0, 16384, 0,
          G_PARAM_READWRITE | G_PARAM_CONSTRUCT));
  g_object_class_install_property (oc, PROP_ALIGN_PROBE,
      g_param_spec_uint ("align-probe", "alignment probe",
          "Samples held on each pad for the delay estimate (0 = 48000 + 2 align-max-lag)", 0, 1 << 20, 0,
          G_PARAM_READWRITE | G_PARAM_CONSTRUCT));
  g_object_class_install_property (oc, PROP_DELAY_WATCH,
      g_param_spec_double ("delay-watch", "delay watch window", "Length of the delay watch's window in seconds (0 = off)", 0,
          1e6, 0, G_PARAM_READWRITE | G_PARAM_CONSTRUCT));
  g_object_class_install_property (oc, PROP_DELAY,
      g_param_spec_int ("delay", "delay", "Delay of the test pad against the reference pad in samples (0 until acquired)",
          -16384, 16384, 0, G_PARAM_READABLE));
  g_object_class_install_property (oc, PROP_DELAY_ACQUIRED,
      g_param_spec_boolean ("delay-acquired", "delay acquired", "The stream's delay has been found", FALSE,
          G_PARAM_READABLE));
  g_object_class_install_property (oc, PROP_DELAY_OFFSET,
      g_param_spec_int ("delay-offset", "delay offset", "Offset the newest window of the delay watch reads, in samples",
          -31, 31, 0, G_PARAM_READABLE));

  gst_element_class_add_static_pad_template (ec, &ref_template);
  gst_element_class_add_static_pad_template (ec, &test_template);
  gst_element_class_set_static_metadata (ec, "Perceptual evaluation of audio quality (MI355X)", "Sink/Audio",
      "Compute objective audio quality measures (ITU-R BS.1387) on an AMD GPU", "gstpeaq_amd");
}

static void
gst_peaq_amd_init (GstPeaqAmd * self)
{
  static GstStaticPadTemplate *tmpl[2] = { &ref_template, &test_template };
  gint i;
  for (i = 0; i < 2; i++) {
    self->pads[i] = gst_pad_new_from_static_template (tmpl[i], i ? "test" : "ref");
    gst_pad_set_chain_function (self->pads[i], gst_peaq_amd_chain);
    gst_pad_set_event_function (self->pads[i], gst_peaq_amd_sink_event);
    gst_pad_set_query_function (self->pads[i], gst_peaq_amd_sink_query);
    gst_element_add_pad (GST_ELEMENT (self), self->pads[i]);
  }
  GST_OBJECT_FLAG_SET (self, GST_ELEMENT_FLAG_SINK);
  self->channels = 0;
  self->rate[0] = self->rate[1] = 0;
  g_queue_init (&self->held[0]);
  g_queue_init (&self->held[1]);
  self->broker_rate[0] = self->broker_rate[1] = 48000;
  self->session = NULL;
  self->broker = NULL;
  self->broker_sid = -1;
  self->failed = FALSE;
  self->pushed = FALSE;
  self->pending_error = NULL;
  self->metered = self->meter_flushed = FALSE;
  self->st_odg = self->st_di = self->st_totalsnr = NAN;
  self->aligning = self->watching = self->delay_acquired = self->watch_seen = FALSE;
  self->delay = self->delay_offset = 0;
}

static gboolean
plugin_init (GstPlugin * plugin)
{
  GST_DEBUG_CATEGORY_INIT (peaq_amd_debug, "peaq", 0, "PEAQ on MI355X");
  return gst_element_register (plugin, "peaq", GST_RANK_NONE, gst_peaq_amd_get_type ());
}

GST_PLUGIN_DEFINE (GST_VERSION_MAJOR, GST_VERSION_MINOR, peaq,
    "Perceptual evaluation of audio quality (ITU-R BS.1387) on AMD MI355X",
    plugin_init, PACKAGE_VERSION, "LGPL", PACKAGE, "https://github.com/HSU-ANT/gstpeaq")
