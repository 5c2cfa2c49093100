#!/usr/bin/env python3
"""CPU simulation of k_map's LDS key table on one workgroup's share of the C2 corpus (4 MiB, ~709 K
tokens): hit rate of the best static table (the most frequent 8,410 short and 1,024 medium keys)
against 2-choice slots with second-sight admission (the kernel's policy) and variants (more
choices, admission on third sight), and of tables seeded before the first token (wcg_seed.h): the
most frequent keys of another 64 MiB of the corpus, SEED_FRAC x slots of each kind offered, placed
greedily (most frequent first, first choice then second, dropped when both are taken); stale seeds
(keys that never occur, or the keys of the seed-43 corpus) the same way.
Usage: tools/hit_sim.py [bytes]   (r06; CPU only, seconds)"""
import os
import sys, re, collections, random
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'mit-6.824-2015_amd'))
from wcg.corpus import Generator, CONFIGS
NS,NM=8410,1024
SEED_BYTES=64<<20          # the text a seed's keys are counted in
SEED_BLOCK=4096            # ... and its first generator block: far from the simulated share's (37)
cfg=CONFIGS['c2_ascii_zipf_1gib']
R=random.Random(1)
hs={}
def H(t):
    h=hs.get(t)
    if h is None: h=hs[t]=R.getrandbits(64)
    return h
def tokens(data):
    toks=re.findall(rb'[A-Za-z]+', data)
    return toks,[t for t in toks if len(t)<=7],[t for t in toks if 8<=len(t)<=15]
def opt(lst,n):
    c=collections.Counter(lst); return sum(v for _,v in c.most_common(n))
def place(keys,n,choices=2):
    """keys (most frequent first) into an empty table of n slots: the table and how many were placed"""
    tab=[None]*n; placed=0
    for t in keys:
        h=H(t)
        for c in [(h>>(i*20))%n for i in range(choices)]:
            if tab[c] is None: tab[c]=t; placed+=1; break
    return tab,placed
def sim(lst,n,choices=2,admit_bits=16384,admit_need=1,tab=None):
    tab=[None]*n if tab is None else list(tab); seen=collections.Counter() if admit_bits else None
    hits=0
    for t in lst:
        h=H(t)
        cand=[(h>>(i*20))%n for i in range(choices)]
        if any(tab[c]==t for c in cand): hits+=1; continue
        free=[c for c in cand if tab[c] is None]
        if not free: continue
        if seen is not None:
            b=(h>>50)%admit_bits
            seen[b]+=1
            if seen[b]<=admit_need: continue
        tab[free[0]]=t; hits+=1
    return hits
def top_keys(corpus_seed,nbytes=SEED_BYTES,first_block=SEED_BLOCK):
    """the short and the medium keys of nbytes of a C2-like corpus, most frequent first"""
    g=Generator(cfg['mode'],cfg['vocab'],cfg['zipf_s'],corpus_seed)
    _,s,m=tokens(g.bytes(nbytes, first_block=first_block))
    return [k for k,_ in collections.Counter(s).most_common()],[k for k,_ in collections.Counter(m).most_common()]
def seeded(short,med,ntok,ks,km,frac):
    """hit rate with the first frac x slots keys of ks / km placed before the first token"""
    ts,ps=place(ks[:int(NS*frac)],NS); tm,pm=place(km[:int(NM*frac)],NM)
    return (sim(short,NS,tab=ts)+sim(med,NM,tab=tm))/ntok,ps,pm
def share(nb=4<<20):
    """one workgroup's share of C2: tokens, short ones, medium ones"""
    g=Generator(cfg['mode'],cfg['vocab'],cfg['zipf_s'],cfg['seed'])
    return tokens(g.bytes(nb, first_block=37))
def seeded_rate(frac,nb=4<<20):
    """the figure DESIGN.md section 22 quotes for a seed of frac x slots (tests/test_hit_sim_seed.py)"""
    toks,short,med=share(nb)
    ks,km=top_keys(cfg['seed'])
    return seeded(short,med,len(toks),ks,km,frac)[0]
def main():
    nb=int(sys.argv[1]) if len(sys.argv)>1 else 4<<20
    toks,short,med=share(nb)
    print('tokens',len(toks))
    print('short',len(short),'med',len(med),'long',len(toks)-len(short)-len(med))
    print('optimal static hits', (opt(short,NS)+opt(med,NM))/len(toks))
    for ch,ab,an in [(2,16384,1),(2,0,0),(4,16384,1),(2,16384,2),(4,16384,2),(8,16384,1)]:
        hsum=sim(short,NS,ch,ab,an)+sim(med,NM,ch,ab,an)
        print('choices',ch,'admit bits',ab,'need',an,'hit',round(hsum/len(toks),4))
    ks,km=top_keys(cfg['seed'])
    for f in (0.5,0.75,0.9,1.0):
        r,ps,pm=seeded(short,med,len(toks),ks,km,f)
        print('seeded',f,'x slots offered, placed',ps,'short',pm,'medium: hit',round(r,4))
    # stale seeds: as many keys, none of which occurs (upper-case copies: C2's words are lower case)
    for f in (1.0,0.75,0.5):
        r,_,_=seeded(short,med,len(toks),[k.upper() for k in ks],[k.upper() for k in km],f)
        print('stale seed (keys that never occur)',f,'x slots offered: hit',round(r,4))
    ks43,km43=top_keys(cfg['seed']+1)
    print('seed-42 and seed-43 vocabularies share',len(set(ks[:NS])&set(ks43[:NS])),'of their top',NS,'short keys')
    print('seed from the seed-43 corpus, 0.75 x slots offered: hit',round(seeded(short,med,len(toks),ks43,km43,0.75)[0],4))
if __name__=='__main__':
    main()
