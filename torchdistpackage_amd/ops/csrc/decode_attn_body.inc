// Body of the first launch of the bf16 decode-attention kernels (grid
// (B*Hkv, nsplit), DA_BLOCK threads): one workgroup, one chunk of keys, all
// M rows of its kv head.  decode_attn.hip describes the design.  The file is
// included inside a kernel template <int D, int MT> whose parameters carry
// the names used below (q, out, part_acc, part_ml, pos_ptr, pos_stride,
// pos_host, Hkv, G, Sq, Smax, chunk, nsplit, q_s*, o_s*, scale_log2).  The
// key source is all the includer varies, through three macros:
//   DA_SRC_INIT()  statements run once per workgroup after the block-uniform
//                  early exit; b, h, ld, c0, c1 and len are in scope
//   DA_KPTR(j)     address of this lane's 16 bytes of key j, c0 <= j < c1
//   DA_VPTR(j)     the same for the value
// so the lane-to-key mapping and the order of every sum and merge are the
// same for every includer.  It is shared as text, not as a template over a
// source functor: that form changed the ISA of all ten contiguous
// instantiations (docs/design/kernels.md, "decode_attn_paged.hip").
  constexpr int LPK = D / 8;          // lanes per key (16 B each)
  constexpr int KPW = WAVE / LPK;     // keys per wave step
  constexpr int KPB = KPW * DA_WAVES; // keys per block step
  constexpr int U = (MT <= 4) ? 4 : 2;  // keys in flight per lane

  __shared__ float sm_acc[DA_WAVES * MT * D];
  __shared__ float sm_ml[DA_WAVES * MT * 2];

  const int bh = blockIdx.x;
  const int b = bh / Hkv, h = bh % Hkv;
  const int split = blockIdx.y;
  const int M = G * Sq;
  const int p0 = da_read_pos(pos_ptr, pos_stride, pos_host, b, Smax, Sq);
  const int len = p0 + Sq;            // <= Smax
  const int c0 = split * chunk;
  if (c0 >= len) return;              // empty split: block-uniform exit
  const int c1 = min(c0 + chunk, len);

  const int wave = threadIdx.x >> 6;
  const int lane = threadIdx.x & 63;
  const int ld = lane % LPK;          // which 8-element slice of the head dim
  const int grp = wave * KPW + lane / LPK;

  uint4 qv[MT];                       // packed bf16, this lane's d-slice
  int rowlim[MT];                     // last visible key of row m
#pragma unroll
  for (int m = 0; m < MT; ++m) {
    qv[m] = make_uint4(0, 0, 0, 0);
    rowlim[m] = -1;                   // padding row: sees nothing
    if (m < M) {
      const int gq = m / Sq, i = m % Sq;
      qv[m] = *(const uint4*)&q[(long)b * q_sb + (long)(h * G + gq) * q_sh +
                                (long)i * q_ss + ld * 8];
      rowlim[m] = p0 + i;
    }
  }

  float mrun[MT], lrun[MT], acc[MT][8];
#pragma unroll
  for (int m = 0; m < MT; ++m) {
    mrun[m] = -INFINITY;
    lrun[m] = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) acc[m][e] = 0.f;
  }

  DA_SRC_INIT();

  // K/V for one step: U keys per lane, 16 B each.  Addresses are clamped
  // into [c0, c1-1], so a lane past the end (and the prefetch past the last
  // step) re-reads the chunk's last key; its score is masked below.
  auto load_kv = [&](int base, uint4 (&kv)[U], uint4 (&vv)[U]) {
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int jc = min(base + u * KPB + grp, c1 - 1);
      kv[u] = *(const uint4*)DA_KPTR(jc);
      vv[u] = *(const uint4*)DA_VPTR(jc);
    }
  };

  // software pipeline: the next step's K/V are requested before this step's
  // arithmetic (up to 16 rows there are registers for it), and the
  // scheduler may not sink the loads down to their first use
  constexpr bool PF = MT <= 8;
  uint4 kv[U], vv[U];
  if (PF) load_kv(c0, kv, vv);
  for (int base = c0; base < c1; base += KPB * U) {
    uint4 kn[PF ? U : 1], vn[PF ? U : 1];
    if constexpr (PF) {
      load_kv(base + KPB * U, kn, vn);
    } else {
      load_kv(base, kv, vv);
    }
    __builtin_amdgcn_sched_barrier(0);
    int jl[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const int j = base + u * KPB + grp;
      jl[u] = (j < c1) ? j : 0x7fffffff;
    }
    float vf[U][8];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      const uint* w = (const uint*)&vv[u];
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        vf[u][2 * e] = __uint_as_float(w[e] << 16);
        vf[u][2 * e + 1] = __uint_as_float(w[e] & 0xffff0000u);
      }
    }
#pragma unroll
    for (int m = 0; m < MT; ++m) {
      const da_sv2* qp = (const da_sv2*)&qv[m];
      float s[U];
      float mn = mrun[m];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const da_sv2* kp = (const da_sv2*)&kv[u];
        float a = 0.f;
#pragma unroll
        for (int e = 0; e < 4; ++e)
          a = __builtin_amdgcn_fdot2_f32_bf16(kp[e], qp[e], a, false);
        a = da_group_sum<LPK>(a);
        s[u] = (jl[u] <= rowlim[m]) ? a * scale_log2 : -INFINITY;
        mn = fmaxf(mn, s[u]);
      }
      // nothing visible yet: keep exp2(-inf - -inf) out of the arithmetic
      const float ms = (mn == -INFINITY) ? 0.f : mn;
      const float alpha = __builtin_amdgcn_exp2f(mrun[m] - ms);
      float p[U], ps = 0.f;
#pragma unroll
      for (int u = 0; u < U; ++u) {
        p[u] = __builtin_amdgcn_exp2f(s[u] - ms);
        ps += p[u];
      }
      mrun[m] = mn;
      lrun[m] = lrun[m] * alpha + ps;
#pragma unroll
      for (int e = 0; e < 8; ++e) {
        float t = acc[m][e] * alpha;
#pragma unroll
        for (int u = 0; u < U; ++u) t = fmaf(p[u], vf[u][e], t);
        acc[m][e] = t;
      }
    }
    if constexpr (PF) {
#pragma unroll
      for (int u = 0; u < U; ++u) {
        kv[u] = kn[u];
        vv[u] = vn[u];
      }
    }
  }

  // merge the lane groups of a wave (each ran its own online softmax)
#pragma unroll
  for (int m = 0; m < MT; ++m) {
    float mx = mrun[m];
#pragma unroll
    for (int off = LPK; off < WAVE; off <<= 1)
      mx = fmaxf(mx, __shfl_xor(mx, off, WAVE));
    const float ms = (mx == -INFINITY) ? 0.f : mx;
    const float f = __builtin_amdgcn_exp2f(mrun[m] - ms);
    float l = lrun[m] * f;
#pragma unroll
    for (int off = LPK; off < WAVE; off <<= 1) l += __shfl_xor(l, off, WAVE);
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      float a = acc[m][e] * f;
#pragma unroll
      for (int off = LPK; off < WAVE; off <<= 1)
        a += __shfl_xor(a, off, WAVE);
      acc[m][e] = a;
    }
    if (lane < LPK) {
#pragma unroll
      for (int e = 0; e < 8; ++e)
        sm_acc[(wave * MT + m) * D + ld * 8 + e] = acc[m][e];
      if (lane == 0) {
        sm_ml[(wave * MT + m) * 2] = mx;
        sm_ml[(wave * MT + m) * 2 + 1] = l;
      }
    }
  }
  __syncthreads();

  // merge the waves; one (row, d) element per thread per trip
  for (int idx = threadIdx.x; idx < M * D; idx += DA_BLOCK) {
    const int m = idx / D, d = idx % D;
    float mx = -INFINITY;
#pragma unroll
    for (int w = 0; w < DA_WAVES; ++w)
      mx = fmaxf(mx, sm_ml[(w * MT + m) * 2]);
    const float ms = (mx == -INFINITY) ? 0.f : mx;
    float l = 0.f, a = 0.f;
#pragma unroll
    for (int w = 0; w < DA_WAVES; ++w) {
      const float f = __builtin_amdgcn_exp2f(sm_ml[(w * MT + m) * 2] - ms);
      l += sm_ml[(w * MT + m) * 2 + 1] * f;
      a += sm_acc[(w * MT + m) * D + d] * f;
    }
    if (nsplit == 1) {
      const int gq = m / Sq, i = m % Sq;
      out[(long)b * o_sb + (long)(h * G + gq) * o_sh + (long)i * o_ss + d] =
          f2bf(a / l);
    } else {
      const long row = ((long)bh * nsplit + split) * MT + m;
      part_acc[row * D + d] = a;
      if (d == 0) {
        part_ml[row * 2] = mx;
        part_ml[row * 2 + 1] = l;
      }
    }
  }
